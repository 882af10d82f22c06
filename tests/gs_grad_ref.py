"""A float64 restatement and a per-element error budget for the 3DGS rasterizer backward (nerficg_amd/csrc/gs_raster.hip: k_render_bw, k_preprocess_bw).
Plain module: no test functions.  Used by tests/test_gs_grad_ref_cpu.py and tests/test_gpu_gs_grad_budget.py.

Stage 1, the restatement of the blend backward (BlendRef)
--------------------------------------------------------
Inputs are a forward state (points_xy, conic_opacity, rgb, point_list, ranges, n_contrib; with the depth / alpha maps also depths), the background and the
pixel gradients.  The float arrays are float32 values promoted to float64; the lists and n_contrib are taken as given -- on the GPU they are the kernel's own
saved state, which the tests hold equal to the f32 oracle's.  For every pixel the blended set is: the list entries in front of n_contrib with power <= 0 and
alpha >= 1/255, both evaluated in float64 (the float32 constants 0.99f and 1.0f / 255.0f promoted).  T_final is the float64 product of (1 - alpha) over that
set -- the kernel's float32 final_T is NOT read.  Each tile's list is then walked back to front, vectorised over the tile's pixels, exactly as
oracle/gs_oracle_impl.h: blend_backward states it:  T <- T / (1 - alpha);  dL/dalpha = T sum_c (c - n_c) g_c - T_final (bg . g) / (1 - alpha);  the addends
    colour_c  alpha T g_c           opacity  G dL/dalpha          with w = o G dL/dalpha:
    mean2D x  -w (dx A + dy B) W/2  mean2D y  -w (dy C + dx B) H/2        conic xx, xy, yy  -w/2 (dx dx, dx dy, dy dy)          dL/dz  alpha T g_d
and n_c <- alpha c + (1 - alpha) n_c.  With the maps, z and 1 are a fourth and fifth channel with background 0 (gs_depth_alpha_ref.py).
Per visible Gaussian and sum q:  S the float64 sum;  A the sum of the addends' magnitudes, every subtraction replaced by a sum of absolute values: c - n by
|c| + |n| with |n| the same recurrence run on |c|, the background term by |T_final| sum_c |bg_c g_c| / (1 - alpha), dx A + dy B by |dx A| + |dy B|;
k the longest chain (blended entries behind and including this one, over its pixels);  the tiles and (tile, 4 x 4 block) pairs with at least one blending
pixel;  n_add the number of addends.  Per tile: gexp, the kernel's fixed-point exponent (below).

Ambiguous pixels.  float32 and float64 can take the two decisions differently where a list entry in front of n_contrib has |255 alpha - 1| < 1e-5 or
|power| < 1e-6 (the float32 error of alpha and power is delta below, 1e-7 .. 1e-6 for the splats of the cases; the power test is taken on both sides of zero).  `mask_ambiguous(g)` zeroes the pixel gradients there
BEFORE they go to either side: such a pixel adds nothing to any sum on either side, and no Gaussian is excused.  The tests cap the masked share at 0.5 %.

The budget of stage 1 (u = 2^-24, gamma(c) = c u / (1 - c u) as in grid_table_grad_ref.py)
---------------------------
    B_q = R_q + gamma(tiles + 2) A_q + fixed_q + tiny_q
R_q = sum over the addends of rel(pixel, entry) |addend|, the addend's magnitude as in A, with
    rel = gamma(n_p + 4 cnt + C1) + Z
  n_p   blended entries of the pixel: the forward's T <- fmaf(-T, alpha, T) (k_render) rounds once per entry, and the backward starts from that final_T;
  cnt   blended entries behind and including this one (<= k): the reciprocal chain `r_om = rcp(1 - alpha_m); T_new = T * r_om` (gradients(), k_render_bw)
        costs per step one rounding for 1 - alpha, v_rcp_f32's 1 ulp = 2 u, one for the product: 4 u;
  C1 = 24: `entry`/`gradients` from the record to the deposited row sum, longest column (mean2D): dx = x - px (used twice: 2), e = c - n (1), the three fmaf of
        dL_dalpha (3; 5 with the maps -- the two extra are inside the margin below), dL_dalpha * T_new (1), neg_tf_bg = -T_final * bg_dot with bg_dot's 3
        roundings and the fmaf that adds it (5), d_op = Gm * dL_dalpha (1), wgt (1), wx / wy (1), fmaf(wx, A, wy * B) (2), the four DPP adds of the
        transposing row reduction (4): 21, plus 3 of margin for the running colour n (one fmaf per entry behind, each of which is also counted in 4 cnt);
  Z = the float32 error of alpha itself, which is NOT a rounding of this chain but of its inputs.  alpha = min(0.99, o G) carries the relative error
        delta = gamma(6) P + gamma(4),  P = (|A| dx^2 + |C| dy^2) / 2 + |B dx dy|  the magnitude of blend_power's terms (six roundings: dx, the packed
        product, two more products, two fmaf), gamma(4) for exp_blend (v_exp_f32 1 ulp, the Cody-Waite products) and o * G.  For the addend of entry k:
        an entry IN FRONT of k enters T as (1 - alpha): relative error alpha delta / (1 - alpha);  k itself enters through G (delta) and, in the background
        term, through r_om (alpha delta / (1 - alpha)): together delta / (1 - alpha);  an entry j BEHIND k has moved the running colour n by
        alpha_j delta_j (c_j - n), which is at most delta_j / (1 - alpha_j) of |n| as the magnitude recurrence carries it; behind entries cancel from T
        exactly (the backward recomputes the forward's alpha bit for bit).  Z(pixel, k) = sum_front alpha delta / (1 - alpha) + sum_{k and behind}
        delta / (1 - alpha).
gamma(tiles + 2) A: the flush of a batch converts the 64-bit sum to float32 (1), multiplies by `inv` (1) and adds it to the Gaussian's record with one float
  atomic per tile (tiles roundings of partial sums, each at most A in magnitude).
fixed_q: `deposit` truncates the scaled row sum toward zero: less than one step 2^(gexp_t - BW_S_class) per depositing (tile t, block) pair (a block whose
  16 pixels all skip the entry deposits exactly 0), times the flush constant `inv` carries: 1 (colour, opacity, dL/dz), W/2, H/2 (mean2D), 1/2 (conic).
  gexp_t = max(BW_E_MIN, frexp exponent of the tile's largest |dL/dpixel|), with the maps of max(|g_rgb|, |g_a|, |g_d| max(1, z_max)), z_max the depth of the
  last entry of the tile's blended prefix (the lines around `frexpf(gmax, &gexp)`).  A tile whose gradients are all zero returns early and deposits nothing.
  (The low word of the conversion is taken from a remainder in [-2^31, 2^31]; a remainder of exactly +2^31 saturates one step short.  That needs a scaled
  sum of at least 2^31 steps, whose own float32 rounding is 64 steps or more: inside gamma(C1)'s margin, not a term of its own.)
tiny_q: the float32 format's lower end -- a product below 2^-126 may be flushed; each of the at most 8 products of an addend loses less than 2^-126 times
  the factors still to come (dx, dy, the conic, the flush constant): 8 * 2^-126 * m_q per addend, m_q = 1 (colour, opacity, dL/dz), o (|dx| + |dy|)
  (|A| + |B| + |C|) W/2 | H/2 (mean2D), o max(dx^2, dy^2) / 2 (conic).  It matters only for gradients near 2^-100.
The serial float32 oracle adds a Gaussian's n_add addends one by one instead: `blend_budget(order='serial')` replaces gamma(tiles + 2) by gamma(n_add) and has no
fixed part.  The relative part (B - fixed - tiny) / A is asserted <= 2e-3, the gate every other 3DGS backward test uses per TENSOR.

Stage 2, the leaves (LeafRef)
-----------------------------
want = oracle.gs_gaussian_backward in float64 on S (the state's cov3D, clamp flags and radii; means, SH, scales, rotations and camera promoted).  Stage 2 is
linear in the sums and Gaussians are independent, so nine further calls with unit vectors give every Gaussian's Jacobian column J_q at once; dL/dz reaches
mean3D through viewmatrix[:3, 2] (gs_depth_alpha_ref.py).
    budget(leaf) = sum_q |J_q| B_q + gamma(C2) sum_q |J_q| |S_q| + cancel(leaf)              A(leaf) = sum_q |J_q| A_q
C2 = 80: the longest chain of preprocess_bw_one, conic -> rotation: t and M = J W (12, used twice: 24), denom (3), denom2inv (3), dL_da (6), o[] (4),
A = R (mod s) with quat_R (7), dA (5), dR (2), g[] (9 terms: 10) = 64, rounded up for the 1-ulp differences of focal_x and the activations.
cancel(leaf): gamma counts roundings RELATIVE to the products it sees; a statement that subtracts nearly equal numbers it has itself rounded needs its
  own term.  Two leaves do:
  The SH gradient is Bv[k] dRGB, and Bv[k] is a polynomial of the unit view direction whose terms cancel (2 zz - xx - yy, xx - yy, ...): its error is
  gamma(C_SH) times the polynomial with every monomial replaced by its absolute value, C_SH = 26: six roundings per direction component (difference, three
  squares and sums, sqrt, divide) times degree three, the monomial's products and sums (5), the constant and the product with dRGB (2).
  dL/dscale[k] = mod sum_r dA[r][k] R[r][k] with dA = 2 Gs A: a double sum of products of either sign, formed from the ROUNDED dL/dcov3D.  Its error is
  gamma(C_SCALE) times the same expression with every product replaced by its absolute value (|Gs| from the float64 dL/dcov3D, whose own error is in the
  terms above), C_SCALE = 14: quat_R (5), A = R (mod s) (2), the three products and two sums of dA (5, the factor 2 exact), those of the dot product
  with R (5) and mod (1), minus what a term shares.  Measured on the f32 oracle: 0.7 of the budget without it at 9 x 5.
A == 0 marks what must be EXACTLY zero: culled Gaussians, visible ones no pixel blended, clamped SH channels, SH coefficients above the active degree,
means2D[:, 2].  `judge` counts every violation.
"""
from __future__ import annotations

import numpy as np

import oracle

U = 2.0 ** -24
TINY = 2.0 ** -126
TILE = 16
BW_S_COLOR, BW_S_OPACITY, BW_S_MEAN, BW_S_CONIC, BW_E_MIN = 51, 39, 40, 25, -60
ALPHA_CAP, ALPHA_MIN = float(np.float32(0.99)), float(np.float32(1.0) / np.float32(255.0))
C1, C2 = 24, 80
QNAMES = ('color0', 'color1', 'color2', 'opacity', 'mean_x', 'mean_y', 'conic_xx', 'conic_xy', 'conic_yy', 'dz')
GATE = 2e-3


def gamma(c):
    c = np.asarray(c, np.float64)
    return c * U / (1.0 - c * U)


# ------------------------------------------------------------------------------------------------------------------------ states
def promote(st, **replace):
    """A float64 oracle state holding st's float32 values (and `replace`'s: arrays of the kernel's saved state) -- what oracle.gs_backward and
    oracle.gs_gaussian_backward take in their double instantiation."""
    f = np.float64
    out = oracle.GSState()
    out.dtype, out.P, out.M, out.D, out.W, out.H = f, st.P, st.M, st.D, st.W, st.H
    for name in ('radii', 'clamped', 'tiles_touched', 'point_list', 'ranges', 'n_contrib'):
        setattr(out, name, np.ascontiguousarray(replace.get(name, getattr(st, name))))
    for name in ('depths', 'points_xy', 'conic_opacity', 'rgb', 'cov3D', 'final_T'):
        a = np.asarray(replace.get(name, getattr(st, name)))
        assert a.dtype == np.float32, name
        setattr(out, name, np.ascontiguousarray(a, f).reshape(getattr(st, name).shape))
    out.num_rendered = st.num_rendered
    out.inputs = {}
    for k, v in st.inputs.items():
        if isinstance(v, np.ndarray):
            out.inputs[k] = np.ascontiguousarray(replace.get(k, v), f)
        elif v is None:
            out.inputs[k] = None
        else:
            out.inputs[k] = float(np.float32(v))                      # tan_fovx, tan_fovy, scale_modifier: the float the f32 side is handed
    return out


# ------------------------------------------------------------------------------------------------------------------------ stage 1
class _Tile:
    pass


class BlendRef:
    """The forward decisions of one state in float64 (constructor), then `sums` per set of pixel gradients."""

    def __init__(self, st, bg, aux=False):
        f = np.float64
        self.W, self.H, self.P, self.aux = int(st.W), int(st.H), int(st.P), bool(aux)
        self.bg = np.asarray(bg, f).reshape(3)
        W, H = self.W, self.H
        gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
        pts, co, rgb = np.asarray(st.points_xy, f), np.asarray(st.conic_opacity, f), np.asarray(st.rgb, f)
        depths = np.asarray(st.depths, f)
        plist, ranges = np.asarray(st.point_list), np.asarray(st.ranges).astype(np.int64)
        ncon = np.asarray(st.n_contrib).astype(np.int64).reshape(H, W)
        self.ambiguous = np.zeros((H, W), bool)
        self.T_final = np.ones((H, W), f)
        self.tiles = []
        for t in range(gx * gy):
            ty, tx = divmod(t, gx)
            ys, xs = np.arange(ty * TILE, min(H, ty * TILE + TILE)), np.arange(tx * TILE, min(W, tx * TILE + TILE))
            py, px = (a.reshape(-1) for a in np.meshgrid(ys, xs, indexing='ij'))
            r0, r1 = ranges[t]
            nc = ncon[py, px]
            assert nc.max(initial=0) <= r1 - r0
            K = int(nc.max(initial=0))
            if K == 0:
                continue
            ids = plist[r0:r0 + K]
            dx, dy = pts[ids, 0, None] - px[None, :], pts[ids, 1, None] - py[None, :]
            A, B, C, o = (co[ids, j, None] for j in range(4))
            power = -0.5 * (A * dx * dx + C * dy * dy) - B * dx * dy
            pmag = 0.5 * (np.abs(A) * dx * dx + np.abs(C) * dy * dy) + np.abs(B * dx * dy)
            G = np.exp(np.minimum(power, 0.0))
            alpha = np.minimum(ALPHA_CAP, o * G)
            front = np.arange(K)[:, None] < nc[None, :]
            active = front & (power <= 0.0) & (alpha >= ALPHA_MIN)
            amb = front & ((np.abs(255.0 * o * G - 1.0) < 1e-5) | (np.abs(power) < 1e-6))
            self.ambiguous[py, px] = amb.any(0)
            al = np.where(active, alpha, 0.0)
            self.T_final[py, px] = np.prod(1.0 - al, axis=0)
            delta = gamma(6) * pmag + gamma(4)
            tl = _Tile()
            tl.t, tl.py, tl.px, tl.ids, tl.dx, tl.dy, tl.G, tl.al, tl.active = t, py, px, ids, dx, dy, G, al, active
            tl.co = co[ids]
            s_front = np.where(active, al * delta / (1.0 - al), 0.0)
            s_here = np.where(active, delta / (1.0 - al), 0.0)
            # entry k: the entries in front of it (exclusive prefix sum) and those behind and including it (inclusive suffix sum)
            tl.Z = (np.cumsum(s_front, 0) - s_front) + np.cumsum(s_here[::-1], 0)[::-1]
            tl.n_p = active.sum(0)
            tl.block = ((py % TILE) // 4) * 4 + (px % TILE) // 4
            ch = [rgb[ids, 0], rgb[ids, 1], rgb[ids, 2]] + ([depths[ids], np.ones(K)] if aux else [])
            tl.c = np.stack(ch, 1)                                     # (K, C)
            tl.z_last = float(np.float32(depths[ids[K - 1]]))
            self.tiles.append(tl)
        self.n_tiles = gx * gy

    def mask_ambiguous(self, g):
        """g (..., H, W) with the ambiguous pixels zeroed (a copy)."""
        g = np.array(g, copy=True)
        g[..., self.ambiguous] = 0
        return g

    def tile_gexp(self, tl, g, g_d=None, g_a=None):
        """(gmax, gexp) of one tile as k_render_bw forms them (float32 arithmetic for the one product)."""
        gmax = np.float32(np.abs(g[:, tl.py, tl.px]).max())
        if self.aux:
            gmax = max(gmax, np.float32(np.abs(g_a[tl.py, tl.px]).max()))
            gmax = max(gmax, np.float32(np.abs(g_d[tl.py, tl.px]).max()) * max(np.float32(1.0), np.float32(tl.z_last)))
        return float(gmax), max(int(np.frexp(np.float64(gmax))[1]), BW_E_MIN)

    def sums(self, g, g_d=None, g_a=None):
        """g (3, H, W) float32 (already masked); with the maps g_d, g_a (H, W).  Returns a dict: S, A, R, tiny (P, NQ) float64; k, tiles, blocks, n_add (P,)
        int64; step (P,) = sum over depositing (tile, block) pairs of 2^gexp_tile; gexp (n_tiles,) int (BW_E_MIN - 1: the tile returns early)."""
        f = np.float64
        NQ = 10 if self.aux else 9
        P, W, H = self.P, self.W, self.H
        g = np.asarray(g)
        assert g.dtype == np.float32 and g.shape == (3, H, W)
        assert not np.asarray(g)[:, self.ambiguous].any(), 'mask the gradients first (mask_ambiguous)'
        if self.aux:
            g_d, g_a = np.asarray(g_d), np.asarray(g_a)
            assert g_d.dtype == g_a.dtype == np.float32 and not g_d[self.ambiguous].any() and not g_a[self.ambiguous].any()
        out = dict(S=np.zeros((P, NQ), f), A=np.zeros((P, NQ), f), R=np.zeros((P, NQ), f), tiny=np.zeros((P, NQ), f), k=np.zeros(P, np.int64),
                   tiles=np.zeros(P, np.int64), blocks=np.zeros(P, np.int64), n_add=np.zeros(P, np.int64), step=np.zeros(P, f),
                   gexp=np.full(self.n_tiles, BW_E_MIN - 1, np.int64))
        S, Am, R, tiny = out['S'], out['A'], out['R'], out['tiny']
        hW, hH = 0.5 * W, 0.5 * H
        bg = self.bg
        for tl in self.tiles:
            gmax, gexp = self.tile_gexp(tl, g, g_d, g_a)
            if not gmax > 0:
                continue
            out['gexp'][tl.t] = gexp
            gv = [g[c, tl.py, tl.px].astype(f) for c in range(3)]
            if self.aux:
                gv += [g_d[tl.py, tl.px].astype(f), g_a[tl.py, tl.px].astype(f)]
            gv = np.stack(gv)                                          # (C, N)
            gabs = np.abs(gv)
            Tf = self.T_final[tl.py, tl.px]
            bgdot, bgabs = (bg[:, None] * gv[:3]).sum(0), np.abs(bg[:, None] * gv[:3]).sum(0)
            N = tl.px.size
            T, cnt = Tf.copy(), np.zeros(N, np.int64)
            n, nabs = np.zeros_like(gv), np.zeros_like(gv)
            step = 2.0 ** gexp
            for k in range(tl.ids.size - 1, -1, -1):
                a = tl.active[k]
                if not a.any():
                    continue
                i = tl.ids[k]
                al, G, dx, dy = tl.al[k], np.where(a, tl.G[k], 0.0), tl.dx[k], tl.dy[k]
                cA, cB, cC, o = tl.co[k]
                r = 1.0 / (1.0 - al)
                T = T * r
                cnt = cnt + a
                c = tl.c[k][:, None]
                e, ea = c - n, np.abs(c) + nabs
                dLda = (e * gv).sum(0) * T - Tf * bgdot * r
                dLda_abs = (ea * gabs).sum(0) * T + Tf * bgabs * r
                w = al * T
                wg, wga = o * G * dLda, np.abs(o) * G * dLda_abs
                add = [w * gv[0], w * gv[1], w * gv[2], G * dLda,
                       -wg * (dx * cA + dy * cB) * hW, -wg * (dy * cC + dx * cB) * hH, -0.5 * wg * dx * dx, -0.5 * wg * dx * dy, -0.5 * wg * dy * dy]
                mag = [w * gabs[0], w * gabs[1], w * gabs[2], G * dLda_abs,
                       wga * (np.abs(dx * cA) + np.abs(dy * cB)) * hW, wga * (np.abs(dy * cC) + np.abs(dx * cB)) * hH, 0.5 * wga * dx * dx,
                       0.5 * wga * np.abs(dx * dy), 0.5 * wga * dy * dy]
                m_mean = np.abs(o) * (np.abs(dx) + np.abs(dy)) * (abs(cA) + abs(cB) + abs(cC))
                m_con = 0.5 * np.abs(o) * np.maximum(dx * dx, dy * dy)
                one = np.ones(N)
                mq = [one, one, one, one, m_mean * hW, m_mean * hH, m_con, m_con, m_con]
                if self.aux:
                    add.append(w * gv[3]); mag.append(w * gabs[3]); mq.append(one)
                add, mag, mq = np.stack(add), np.stack(mag), np.stack(mq)
                rel = gamma(tl.n_p + 4 * cnt + C1) + tl.Z[k]
                S[i] += add.sum(1)
                Am[i] += mag.sum(1)
                R[i] += (mag * rel[None, :]).sum(1)
                tiny[i] += 8 * TINY * (mq * a[None, :]).sum(1)
                out['k'][i] = max(out['k'][i], int(cnt[a].max()))
                out['tiles'][i] += 1
                nb = np.unique(tl.block[a]).size
                out['blocks'][i] += nb
                out['n_add'][i] += int(a.sum())
                out['step'][i] += nb * step
                n = n + al * e
                nabs = al * np.abs(c) + (1.0 - al) * nabs
        return out


def blend_budget(ref, W, H, order='kernel'):
    """B (P, NQ) of the docstring from BlendRef.sums' dict."""
    NQ = ref['S'].shape[1]
    A = ref['A']
    if order == 'serial':
        B = ref['R'] + gamma(ref['n_add'])[:, None] * A + ref['tiny']
        rel = B - ref['tiny']
    else:
        fixed = np.empty_like(A)
        const = [2.0 ** -BW_S_COLOR] * 3 + [2.0 ** -BW_S_OPACITY] + [0.5 * W * 2.0 ** -BW_S_MEAN, 0.5 * H * 2.0 ** -BW_S_MEAN] + [0.5 * 2.0 ** -BW_S_CONIC] * 3 + [2.0 ** -BW_S_COLOR]
        for q in range(NQ):
            fixed[:, q] = ref['step'] * const[q]
        relp = ref['R'] + gamma(ref['tiles'] + 2)[:, None] * A
        B = relp + fixed + ref['tiny']
        rel = relp
    assert (rel <= GATE * A).all(), 'the relative part of the budget exceeds the 2e-3 gate'
    return B


# ------------------------------------------------------------------------------------------------------------------------ stage 2
def _sums_to_inputs(X, P):
    """(P, NQ) column layout -> the four arrays gs_gaussian_backward takes."""
    mean2D, conic = np.zeros((P, 3)), np.zeros((P, 4))
    mean2D[:, 0], mean2D[:, 1] = X[:, 4], X[:, 5]
    conic[:, 0], conic[:, 1], conic[:, 3] = X[:, 6], X[:, 7], X[:, 8]
    return mean2D, conic, X[:, 3].copy(), X[:, :3].copy()


LEAVES = ('mean3D', 'cov3D', 'sh', 'scale', 'rot')


_SH_C0, _SH_C1 = 0.28209479177387814, 0.4886025119029199
_SH_C2 = (1.0925484305920792, 1.0925484305920792, 0.31539156525252005, 1.0925484305920792, 0.5462742152960396)
_SH_C3 = (0.5900435899266435, 2.890611442640554, 0.4570457994644658, 0.3731763325901154, 0.4570457994644658, 1.445305721320277, 0.5900435899266435)
C_SH = 26


def _sh_basis_magnitude(st64):
    """(P, 16): the SH basis values Bv[k] of preprocess_bw_one with every monomial replaced by its absolute value (the constants are |SH_C*|)."""
    a = st64.inputs
    d = a['means3D'] - a['campos'][None, :]
    with np.errstate(all='ignore'):
        x, y, z = (np.abs(d / np.sqrt((d * d).sum(1))[:, None])).T
    xx, yy, zz = x * x, y * y, z * z
    c, e = _SH_C2, _SH_C3
    out = [np.full_like(x, _SH_C0), _SH_C1 * y, _SH_C1 * z, _SH_C1 * x,
           c[0] * x * y, c[1] * y * z, c[2] * (2 * zz + xx + yy), c[3] * x * z, c[4] * (xx + yy),
           e[0] * y * (3 * xx + yy), e[1] * x * y * z, e[2] * y * (4 * zz + xx + yy), e[3] * z * (2 * zz + 3 * xx + 3 * yy), e[4] * x * (4 * zz + xx + yy),
           e[5] * z * (xx + yy), e[6] * x * (xx + 3 * yy)]
    return np.nan_to_num(np.stack(out, 1))


C_SCALE = 14


def _scale_magnitude(st64, dcov):
    """(P, 3): dL_dscale of preprocess_bw_one with every product replaced by its absolute value, from the float64 dL/dcov3D (P, 6)."""
    a = st64.inputs
    r, x, y, z = a['rotations'].T
    Rm = np.abs(np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                          2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3))
    mod = a['scale_modifier']
    Am = Rm * (mod * np.abs(a['scales']))[:, None, :]
    o = np.abs(dcov)
    Gs = np.stack([o[:, 0], 0.5 * o[:, 1], 0.5 * o[:, 2], 0.5 * o[:, 1], o[:, 3], 0.5 * o[:, 4], 0.5 * o[:, 2], 0.5 * o[:, 4], o[:, 5]], 1).reshape(-1, 3, 3)
    dA = 2 * np.einsum('prj,pjk->prk', Gs, Am)
    return mod * (dA * Rm).sum(1)


class LeafRef:
    """want / budget / A for every leaf, in the oracle's names (mean3D, mean2D, opacity, color, conic, cov3D, sh, scale, rot)."""

    def __init__(self, st64, ref, B, view_z=None):
        P = st64.P
        S, A = ref['S'], ref['A']
        NQ = S.shape[1]
        self.want = oracle.gs_gaussian_backward(st64, *_sums_to_inputs(S, P))
        bud = {k: np.zeros_like(self.want[k]) for k in LEAVES}
        mag = {k: np.zeros_like(self.want[k]) for k in LEAVES}
        lin = {k: np.zeros_like(self.want[k]) for k in LEAVES}

        def col(v):                                                  # (P,) against a leaf of any rank
            return lambda leaf: v.reshape((P,) + (1,) * (leaf.ndim - 1))

        for q in (0, 1, 2, 4, 5, 6, 7, 8):
            X = np.zeros((P, NQ))
            X[:, q] = 1.0
            J = oracle.gs_gaussian_backward(st64, *_sums_to_inputs(X, P))
            for k in LEAVES:
                aj = np.abs(J[k])
                bud[k] += aj * col(B[:, q])(aj)
                mag[k] += aj * col(A[:, q])(aj)
                lin[k] += aj * col(np.abs(S[:, q]))(aj)
        for k in LEAVES:
            bud[k] += gamma(C2) * lin[k]
        if st64.inputs['shs'] is not None:                           # cancel(sh): the basis polynomials
            nb = (st64.D + 1) ** 2
            live = (np.asarray(st64.radii) > 0)[:, None] & (np.asarray(st64.clamped) == 0)
            bud['sh'][:, :nb] += gamma(C_SH) * _sh_basis_magnitude(st64)[:, :nb, None] * (np.abs(S[:, :3]) * live)[:, None, :]
        if st64.inputs['scales'] is not None:                        # cancel(scale): the column dot products dA . R
            bud['scale'] += gamma(C_SCALE) * _scale_magnitude(st64, self.want['cov3D'])
        if NQ == 10:                                                 # dL/dz -> mean3D through viewmatrix[:3, 2], visible Gaussians only
            vz = np.abs(np.asarray(view_z, np.float64).reshape(1, 3)) * (np.asarray(st64.radii) > 0)[:, None]
            self.want['mean3D'] = self.want['mean3D'] + np.asarray(view_z, np.float64).reshape(1, 3) * S[:, 9, None] * (np.asarray(st64.radii) > 0)[:, None]
            bud['mean3D'] += vz * (B[:, 9, None] + gamma(2) * np.abs(S[:, 9, None]))
            mag['mean3D'] += vz * A[:, 9, None]
        m2, con, op, colr = _sums_to_inputs(S, P)
        b2, bcon, bop, bcol = _sums_to_inputs(B, P)
        a2, acon, aop, acol = _sums_to_inputs(A, P)
        self.want.update(mean2D=m2, conic=con, opacity=op, color=colr)
        bud.update(mean2D=b2, conic=bcon, opacity=bop, color=bcol)
        mag.update(mean2D=a2, conic=acon, opacity=aop, color=acol)
        self.budget, self.A = bud, mag

    def to_raw_parameters(self, o, s, q_hat, q_norm):
        """The leaves of a raw_parameters call: opacity -> logit (x o (1 - o)), scale -> log-scale (x s), rot -> the unnormalised quaternion
        ((g - q^ (q^ . g)) / |q|), as the last lines of preprocess_bw_one chain them.  o (P,), s (P, 3), q_hat (P, 4): the float32 activations both sides
        use, promoted; q_norm (P,): |q| of the raw quaternion.  Roundings: 1 - o and two products (3); one product (1); the dot product, the product with
        q^, the difference and the division (4 + 3 = 7, taken relative to |g| + |q^| (|q^| . |g|))."""
        f = np.float64
        o, s, q_hat, q_norm = (np.asarray(a, f) for a in (o, s, q_hat, q_norm))
        w, b, a = self.want, self.budget, self.A
        d = o * (1.0 - o)
        w['opacity'], a['opacity'] = w['opacity'] * d, a['opacity'] * d
        b['opacity'] = b['opacity'] * d + gamma(3) * np.abs(w['opacity'])
        w['scale'], a['scale'] = w['scale'] * s, a['scale'] * s
        b['scale'] = b['scale'] * s + gamma(1) * np.abs(w['scale'])
        g = w['rot']
        aq = np.abs(q_hat)
        spread = lambda v: (v + aq * (aq * v).sum(1, keepdims=True)) / q_norm[:, None]
        w['rot'] = (g - q_hat * (q_hat * g).sum(1, keepdims=True)) / q_norm[:, None]
        b['rot'] = spread(b['rot']) + gamma(7) * spread(np.abs(g))
        a['rot'] = spread(a['rot'])


def judge(got, want, budget, A):
    """(worst err / budget over the elements with A > 0, number of elements over budget, number of A == 0 elements that are not exactly zero)."""
    got = np.asarray(got, np.float64).reshape(want.shape)
    live = A > 0
    err = np.abs(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(live, err / budget, 0.0)
    bad = live & ~(err <= budget)                                    # (a NaN or inf is over budget)
    return float(ratio.max(initial=0.0)) if np.isfinite(ratio).all() else float('inf'), int(bad.sum()), int((~live & (got != 0)).sum())
