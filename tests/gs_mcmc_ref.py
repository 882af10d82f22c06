"""TEST INFRASTRUCTURE ONLY: the f64 statement of 3DGS-MCMC (Kheradmand et al., "3D Gaussian Splatting as Markov Chain Monte Carlo", NeurIPS 2024) as
include/nerficg_hip.h group 16 specifies it -- the yardstick of csrc/gs_mcmc.hip and of the host logic in nerficg_amd.gaussian_splatting.

    A  relocation        relocation_ref, denom_double_sum (the literal double sum), denom_collapsed (what the kernel evaluates)
    B  SGLD noise        noise_ref (+ its per-element budget, + three mutants), noise_torch (the published tensor expression, for tools/bench_gs_mcmc.py),
                         generator_words / box_muller (Philox4x32-10 on tests/philox_ref.py)
    C  regularisers      regulariser_ref
    D  host logic        relocate_plain / add_new_plain on plain numpy arrays

Raw parameters as Gaussians stores them: o = sigmoid(logit), s = exp(log_scale), q = rotation / max(|rotation|, 1e-12) (real part first), R = R(q).
Inputs are the f32 values the kernel reads, taken to f64 exactly; everything after that is f64.
"""
import math

import numpy as np

from tests import philox_ref

N_MAX = 50
O_MIN, O_MAX = 0.005, 1.0 - 2.0 ** -24
BINOM = np.array([[float(math.comb(n, k)) if k <= n else 0.0 for k in range(N_MAX + 1)] for n in range(N_MAX + 1)])   # exact: C(50, 25) < 2^53


# ---------------------------------------------------------------------------------------------------------------- A: relocation
def denom_double_sum(o_new: float, n: int) -> float:
    """sum_{i=1..N} sum_{k=0..i-1} C(i-1, k) (-1)^k / sqrt(k+1) o_new^(k+1), the specification's double sum, term by term."""
    return math.fsum(BINOM[i - 1, k] * (-1.0) ** k / math.sqrt(k + 1.0) * o_new ** (k + 1) for i in range(1, n + 1) for k in range(i))


def denom_collapsed(o_new: float, n: int) -> float:
    """The same sum with the inner sums over i collapsed by sum_{i=k+1..N} C(i-1, k) = C(N, k+1) (hockey stick): N terms."""
    return math.fsum(BINOM[n, k + 1] * (-1.0) ** k / math.sqrt(k + 1.0) * o_new ** (k + 1) for k in range(n))


def copies(count):
    """N = clamp(count + 1, 1, 50)"""
    return np.clip(np.asarray(count, dtype=np.int64) + 1, 1, N_MAX)


def relocation_one(logit: float, n: int):
    """(o, o_new before the clamp, denom) of one Gaussian of logit `logit` that stands for n copies.  1 - o and its n-th root through log1p / expm1:
    the literal 1 - (1 - o)^(1/N) would cancel for o near 1."""
    o = 1.0 / (1.0 + math.exp(-logit))
    log_1mo = -(max(logit, 0.0) + math.log1p(math.exp(-abs(logit))))      # ln(1 - o) = -ln(1 + e^logit)
    o_new = -math.expm1(log_1mo / n)
    return o, o_new, denom_double_sum(o_new, n)


def relocation_ref(logits, log_scales, count):
    """Step A on every row with count > 0 (the others keep their values): dict of f64 arrays 'logit' (P), 'log_scale' (P, 3), 'opacity' (P, the clamped
    o_new), 'scale' (P, 3, s_new), 'ratio' (P, o / denom), 'clamped' (P; -1 / 0 / +1: which end of the clamp was hit)."""
    l = np.asarray(logits, dtype=np.float64).reshape(-1)
    ls = np.asarray(log_scales, dtype=np.float64).reshape(-1, 3)
    cnt = np.asarray(count).reshape(-1)
    n = copies(cnt)
    out = {'logit': l.copy(), 'log_scale': ls.copy(), 'opacity': 1.0 / (1.0 + np.exp(-l)), 'scale': np.exp(ls), 'ratio': np.ones_like(l),
           'clamped': np.zeros(l.shape, dtype=np.int64)}
    for i in np.nonzero(cnt > 0)[0]:
        o, o_new, denom = relocation_one(float(l[i]), int(n[i]))
        ratio = o / denom
        oc = min(max(o_new, O_MIN), O_MAX)
        out['clamped'][i] = -1 if o_new < O_MIN else (1 if o_new > O_MAX else 0)
        out['opacity'][i] = oc
        out['logit'][i] = math.log(oc / (1.0 - oc))
        out['ratio'][i] = ratio
        out['scale'][i] = ratio * np.exp(ls[i])
        out['log_scale'][i] = np.log(ratio * np.exp(ls[i]))
    return out


# ---------------------------------------------------------------------------------------------------------------- B: noise
def rotation_parts(rotations):
    """R (P, 3, 3) of the normalised quaternions, and M (P, 3, 3): per entry the summed magnitude of the products 2 q_a q_b it is formed from (the constant
    1 of the diagonal is not one of them) -- what an entry's rounding error is proportional to when its products cancel."""
    q = np.asarray(rotations, dtype=np.float64).reshape(-1, 4)
    q = q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-12)
    r, i, j, k = q.T
    ii, jj, kk, ij, ik, jk, ri, rj, rk = 2 * i * i, 2 * j * j, 2 * k * k, 2 * i * j, 2 * i * k, 2 * j * k, 2 * r * i, 2 * r * j, 2 * r * k
    R = np.stack([np.stack([1 - (jj + kk), ij - rk, ik + rj], -1), np.stack([ij + rk, 1 - (ii + kk), jk - ri], -1), np.stack([ik - rj, jk + ri, 1 - (ii + jj)], -1)], 1)
    a = np.abs
    M = np.stack([np.stack([jj + kk, a(ij) + a(rk), a(ik) + a(rj)], -1), np.stack([a(ij) + a(rk), ii + kk, a(jk) + a(ri)], -1),
                  np.stack([a(ik) + a(rj), a(jk) + a(ri), ii + jj], -1)], 1)
    return R, M


BUDGET_B0 = 11.0     # roundings along an addend outside the rotation entries, in units of 2^-23 (see noise_ref)
BUDGET_C = 3.0       # the gate's conditioning on the f32 opacity: c * 100 * o


def noise_ref(positions, rotations, log_scales, logits, z, lr, noise_lr=5e5, mutant=None):
    """Step B: (x', budget, gate), all f64, x' and budget (P, 3).

        gate = 1 / (1 + exp(-100 ((1 - o) - 0.995)));   v = z gate (noise_lr lr);   x' = x + R diag(s^2) R^T v
        (noise_lr and lr as the f32 values the kernel receives, their product rounded to f32 like the kernel's).

    mutant: None, or one of three wrong kernels -- 'scale' (diag(s) for diag(s^2)), 'transpose' (R^T ... R for R ... R^T), 'gate' (the gate taken at o, not 1 - o).

    The budget of element i of a row, for a kernel that evaluates the expression in f32 with one rounding per operation (compiled without contraction):

        2^-24 |x'_i|  +  2^-23 sum_jk [ (B0 + c 100 o) |R_ik| |R_jk| + E_ik |R_jk| + |R_ik| E_jk ] s_k^2 |v_j|

    that is the form (B + c 100 o) 2^-23 sum_jk |R_ik| s_k^2 |R_jk| |v_j| with the rounding count B of an addend split into B0, the same for every
    addend, and the share of the two rotation entries it passes through, E / |R|, which is NOT the same for every addend: an entry is a sum of two
    products that can cancel, so its error is proportional to the products' magnitudes M, not to |R|.  Counted in u = 2^-24 (the relative error bound
    of one correctly rounded operation; expf is taken at 1 ulp = 2 u, HIP's documented bound), first order, 2^-23 = 2 u:

      final add x + d                                          the first term, half an ulp of the result
      o = 1 / (1 + expf(-logit))                               2 u (expf, damped by e / (1 + e) <= 1) + 1 u + 1 u = 4 u
      a = 100 (0.005f - o)   [= 100 ((1 - o) - 0.995)]         |da| <= 100 (4 u o + 0.005 u + u |0.005 - o|) + u |a| <= 600 o u + 1.5 u
      gate = 1 / (1 + expf(-a))                                d gate / gate = (1 - gate) da <= da, + 2 u + 1 u + 1 u           -> 5.5 u + 600 o u
      v_j = (z_j gate) (noise_lr lr)                           1 u + 1 u + 1 u (the product of the two rates)                  -> 8.5 u + 600 o u
      s_k^2 = expf(log_scale)^2                                2 u twice + 1 u                                                  -> 5 u
      t_k = sum_j R_jk v_j,  u_k = s_k^2 t_k,  d_i = sum_k R_ik u_k     1 u per product (three), 2 u per three-term sum (two; relative to the sum of magnitudes) -> 7 u
                                                               total 20.5 u = 10.25 x 2^-23: B0 = 11;  600 o u = 300 o x 2^-23: c = 3
      q / |q|: squares 1 u, three adds of positive terms 1 u each -> 4 u, sqrt halves it and adds 1 u -> 3 u, the division 1 u: 4 u per component
      2 q_a q_b: 8 u + 1 u = 9 u;  an entry a +- b, or 1 - (a + b): <= 10 u (|a| + |b|) + 1 u |R| = (5 M + 0.5 |R|) x 2^-23 = E
    """
    x = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    l = np.asarray(logits, dtype=np.float64).reshape(-1)
    s = np.exp(np.asarray(log_scales, dtype=np.float64).reshape(-1, 3))
    zz = np.asarray(z, dtype=np.float64).reshape(-1, 3)
    o = 1.0 / (1.0 + np.exp(-l))
    R, M = rotation_parts(rotations)
    arg = 100.0 * (((1.0 - o) if mutant != 'gate' else o) - 0.995)
    gate = 1.0 / (1.0 + np.exp(-arg))
    step = float(np.float32(np.float32(noise_lr) * np.float32(lr)))
    v = zz * gate[:, None] * step
    d = (s if mutant == 'scale' else s * s)
    if mutant == 'transpose':
        moved = np.einsum('pki,pk,pkj,pj->pi', R, d, R, v)
    else:
        moved = np.einsum('pik,pk,pjk,pj->pi', R, d, R, v)
    x_new = x + moved
    aR, av = np.abs(R), np.abs(v)
    E = 5.0 * M + 0.5 * aR
    w = s * s                                                            # (P, k)
    col = np.einsum('pjk,pj->pk', aR, av)                                # sum_j |R_jk| |v_j|
    col_e = np.einsum('pjk,pj->pk', E, av)                               # sum_j E_jk |v_j|
    common = (BUDGET_B0 + BUDGET_C * 100.0 * o)[:, None] * np.einsum('pik,pk->pi', aR, w * col)
    entries = np.einsum('pik,pk->pi', E, w * col) + np.einsum('pik,pk->pi', aR, w * col_e)
    budget = 2.0 ** -24 * np.abs(x_new) + 2.0 ** -23 * (common + entries)
    return x_new, budget, gate


def noise_torch(positions, rotations, log_scales, logits, z, lr, noise_lr=5e5):
    """Step B as the published implementation writes it with tensor operations ((P, 3, 3) temporaries, ~20 launches), in the dtype of its inputs: the
    comparison partner of the kernel in tools/bench_gs_mcmc.py.  Returns the new positions."""
    import torch
    q = torch.nn.functional.normalize(rotations, dim=-1)
    r, i, j, k = q.unbind(-1)
    R = torch.stack([1 - 2 * (j * j + k * k), 2 * (i * j - r * k), 2 * (i * k + r * j),
                     2 * (i * j + r * k), 1 - 2 * (i * i + k * k), 2 * (j * k - r * i),
                     2 * (i * k - r * j), 2 * (j * k + r * i), 1 - 2 * (i * i + j * j)], dim=-1).reshape(-1, 3, 3)
    L = R * torch.exp(log_scales)[:, None, :]
    covariance = L @ L.transpose(1, 2)
    gate = torch.sigmoid(100.0 * ((1.0 - torch.sigmoid(logits.reshape(-1, 1))) - 0.995))
    noise = z * gate * (noise_lr * lr)
    return positions + torch.bmm(covariance, noise[:, :, None]).squeeze(-1)


def generator_words(seed: int, iteration: int, index):
    """The four Philox4x32-10 words of global row `index`: counter = (index lo, index hi, iteration lo, iteration hi), key = (seed lo, seed hi)."""
    index = np.asarray(index, dtype=np.uint64)
    lo = lambda v: np.asarray(v, dtype=np.uint64) & np.uint64(0xffffffff)
    hi = lambda v: np.asarray(v, dtype=np.uint64) >> np.uint64(32)
    it, sd = np.uint64(iteration), np.uint64(seed)
    return philox_ref.philox4x32_10((lo(index), hi(index), np.broadcast_to(lo(it), index.shape), np.broadcast_to(hi(it), index.shape)), (lo(sd), hi(sd)))


def box_muller(words):
    """(P, 3) f64 normals of the four words: ua = ((w0 >> 8) + 1) 2^-24, ub = (w1 >> 8) 2^-24, uc = ((w2 >> 8) + 1) 2^-24, ud = (w3 >> 8) 2^-24;
    z0 = sqrt(-2 ln ua) cos(2 pi ub), z1 = sqrt(-2 ln ua) sin(2 pi ub), z2 = sqrt(-2 ln uc) cos(2 pi ud)."""
    w = [np.asarray(x, dtype=np.uint32) >> np.uint32(8) for x in words]
    ua, ub = (w[0].astype(np.float64) + 1.0) * 2.0 ** -24, w[1].astype(np.float64) * 2.0 ** -24
    uc, ud = (w[2].astype(np.float64) + 1.0) * 2.0 ** -24, w[3].astype(np.float64) * 2.0 ** -24
    ra, rc = np.sqrt(-2.0 * np.log(ua)), np.sqrt(-2.0 * np.log(uc))
    return np.stack([ra * np.cos(2 * np.pi * ub), ra * np.sin(2 * np.pi * ub), rc * np.cos(2 * np.pi * ud)], -1)


LR_POSITIONS = 0.00016      # LEARNING_RATE_POSITION_INIT at camera extent 1
NOISE_OPACITIES = (0.001, 0.004, 0.005, 0.01, 0.03, 0.06, 0.2, 0.9, 0.999)


def logit32(o):
    o = np.asarray(o, dtype=np.float64)
    return np.log(o / (1.0 - o)).astype(np.float32)


def noise_inputs(P: int, seed: int = 0):
    """The f32 inputs of the noise tests (tests/test_gpu_gs_mcmc.py, and the mutant check on the CPU): positions in [-2, 2]^3; quaternions of any
    length (generic rotations, so R ... R^T and R^T ... R differ); scales anisotropic by a factor of up to 4 per axis around a base that spans
    3e-3 ... 3 over the rows (so diag(s) and diag(s^2) differ, and the step stands far above an ulp of the position); opacities cycling through
    NOISE_OPACITIES: full steps (o <= 0.005), the gate's slope, and closed gates (o >= 0.9: gate < 1e-30)."""
    rng = np.random.default_rng(1000 + seed)
    x = rng.uniform(-2.0, 2.0, (P, 3)).astype(np.float32)
    q = (rng.standard_normal((P, 4)) * rng.uniform(0.5, 2.0, (P, 1))).astype(np.float32)
    base = np.exp(rng.uniform(np.log(3e-3), np.log(3.0), (P, 1)))
    axes = np.stack([rng.permutation(3) for _ in range(P)]).astype(np.float64)           # 0, 1, 2 in random order: factors 1, 2, 4
    ls = np.log(base * 2.0 ** axes * rng.uniform(0.9, 1.1, (P, 3))).astype(np.float32)
    logit = logit32(np.asarray(NOISE_OPACITIES)[np.arange(P) % len(NOISE_OPACITIES)]).reshape(P, 1)
    z = rng.standard_normal((P, 3)).astype(np.float32)
    return {'positions': x, 'rotations': q, 'log_scales': ls, 'logits': logit, 'z': z, 'lr': LR_POSITIONS}


RELOC_OPACITIES = (0.005, 0.0050001, 0.1, 0.5, 0.9, 0.99, 0.999, 1.0 - 2.0 ** -24)
RELOC_COUNTS = (0, 1, 2, 6, 49, 50, 80)


def relocation_inputs(P: int = 4099, seed: int = 0):
    """The f32 inputs of the relocation test: opacities cycling through RELOC_OPACITIES (8) and counts through RELOC_COUNTS (7): every pair occurs;
    scales log-uniform in 1e-4 ... 10.  The last three rows carry logits 40, 60 and 88 with counts 1, 2, 1: there 1 - (1 - o)^(1/N) lies above
    1 - 2^-24, the upper end of the clamp (no opacity that f32 sigmoid can return reaches it with N >= 2)."""
    rng = np.random.default_rng(2000 + seed)
    logit = logit32(np.asarray(RELOC_OPACITIES)[np.arange(P) % len(RELOC_OPACITIES)])
    count = np.asarray(RELOC_COUNTS, dtype=np.int32)[np.arange(P) % len(RELOC_COUNTS)].copy()
    logit[-3:] = (40.0, 60.0, 88.0)
    count[-3:] = (1, 2, 1)
    ls = rng.uniform(np.log(1e-4), np.log(10.0), (P, 3)).astype(np.float32)
    return {'logits': logit.reshape(P, 1), 'log_scales': ls, 'count': count}


# ---------------------------------------------------------------------------------------------------------------- C: regularisers
def regulariser_ref(logits, log_scales, opacity_reg=0.01, scale_reg=0.01):
    """(d L_o / d logit (P), d L_s / d log_scale (P, 3), L_o, L_s): L_o = opacity_reg mean(o), L_s = scale_reg mean(s)."""
    l = np.asarray(logits, dtype=np.float64).reshape(-1)
    s = np.exp(np.asarray(log_scales, dtype=np.float64).reshape(-1, 3))
    P = l.shape[0]
    e = np.exp(-np.abs(l))
    o = np.where(l >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    return opacity_reg / P * e / (1.0 + e) ** 2, scale_reg / (3.0 * P) * s, opacity_reg * math.fsum(o) / P, scale_reg * math.fsum(s.reshape(-1)) / (3.0 * P)


# ---------------------------------------------------------------------------------------------------------------- D: host logic
PARAMS = ('positions', 'f_dc', 'f_rest', 'opacities', 'scales', 'rotations')


def _apply_relocation(model, count):
    ref = relocation_ref(model['opacities'], model['scales'], count)
    hit = np.asarray(count) > 0
    model['opacities'][hit] = ref['logit'][hit].astype(np.float32)[:, None]
    model['scales'][hit] = ref['log_scale'][hit].astype(np.float32)
    for name in PARAMS:
        for m in ('exp_avg', 'exp_avg_sq'):
            model[m][name][hit] = 0.0


def relocate_plain(model, drawn, min_opacity=0.005):
    """D.relocate on a dict of numpy arrays: the six parameters under PARAMS and the moments under 'exp_avg' / 'exp_avg_sq' (dicts by the same names).
    `drawn`: the rows that were drawn for the dead rows, in order.  Returns (dead rows, moved?)."""
    o = 1.0 / (1.0 + np.exp(-model['opacities'].astype(np.float64).reshape(-1)))
    dead = np.nonzero(o <= min_opacity)[0]
    if dead.size == 0 or dead.size == o.size:
        return dead, False
    drawn = np.asarray(drawn, dtype=np.int64)
    assert drawn.size == dead.size
    _apply_relocation(model, np.bincount(drawn, minlength=o.size))
    for name in PARAMS:
        model[name][dead] = model[name][drawn]
    return dead, True


def growth(P: int, cap_max: int) -> int:
    return max(0, min(cap_max, int(1.05 * P)) - P)


def add_new_plain(model, drawn, cap_max):
    """D.add_new on the same dict; `drawn`: the growth(P, cap_max) drawn rows.  Returns n."""
    P = model['positions'].shape[0]
    n = growth(P, cap_max)
    if n == 0:
        return 0
    drawn = np.asarray(drawn, dtype=np.int64)
    assert drawn.size == n
    _apply_relocation(model, np.bincount(drawn, minlength=P))
    for name in PARAMS:
        model[name] = np.concatenate([model[name], model[name][drawn]])
        for m in ('exp_avg', 'exp_avg_sq'):
            model[m][name] = np.concatenate([model[m][name], np.zeros_like(model[m][name][drawn])])
    return n
