"""nerficg_amd.apex_optimizers -- drop-in for `apex.optimizers.FusedAdam` as nerficg imports it (src/Thirdparty/Apex.py:17) and builds
it (src/Methods/InstantNGP/Trainer.py:33-38; src/Methods/GaussianSplatting/Model.py:131-136): FusedAdam(params | param_groups, lr, eps,
betas, adam_w_mode, weight_decay, bias_correction).

* state per parameter = {'exp_avg', 'exp_avg_sq'} (same names as apex / torch.optim.Adam), the step counter lives in the parameter
  group like in apex -- so the reference's optimizer-state surgery (src/Optim/adam_utils.py:6-98: prune / extend / sort / reset of
  single-parameter groups) works unchanged;
* `_step_supports_amp_scaling`: torch.amp.GradScaler hands over its scale and found-inf tensors and the kernel applies them on the
  device (apex's FusedAdam makes the scaler unscale in a separate pass and sync on found_inf).  With apex an overflow-skipped step does not
  advance the step counter (the scaler never calls step()); here `group['step']` is advanced on the host every call and a device counter
  of skipped steps is subtracted inside nrc_adam_prepare, so the bias corrections follow the reference's trajectory without a host sync
  (`effective_step(group)` reads the corrected count back);
* `capturable=True` (apex's flag for graph capture): group['step'] is a device int32 that the kernel advances itself and the learning rate is
  read from a device scalar per group, so a step recorded in a HIP graph (nerficg_amd.graphs) keeps counting on replay; after changing
  group['lr'] (a scheduler) call `sync_hyperparameters()` between replays;
* a parameter that belongs to a nerficg_amd.tinycudann module gets its fp16 compute copy rewritten by the same kernel and its version
  counter bumped, so the next forward can neither see stale weights nor pay a separate conversion pass;
* `step(visibility=mask)` (not in apex; 3DGS `sparse_adam`, gsplat `SelectiveAdam`): rows that the (P,) mask calls invisible keep their values and
  both moments, the other rows get the same update as in the dense step (nerficg_amd/csrc/adam_rows.hip, group 24).
Kernel: nerficg_amd/csrc/adam.hip through the C ABI (include/nerficg_hip.h group 8).
"""
from __future__ import annotations

import ctypes
import weakref

import torch

from .. import _lib

__all__ = ['FusedAdam']


class FusedAdam(torch.optim.Optimizer):
    _step_supports_amp_scaling = True

    def __init__(self, params, lr=1e-3, bias_correction=True, betas=(0.9, 0.999), eps=1e-8, adam_w_mode=True, weight_decay=0.0, amsgrad=False,
                 capturable=False, master_weights=False, set_grad_none=True):
        if amsgrad:
            raise RuntimeError('FusedAdam does not support the AMSGrad variant.')  # same restriction as apex
        if master_weights:
            raise RuntimeError('nerficg_amd FusedAdam: master_weights is not implemented')
        defaults = dict(lr=lr, bias_correction=bias_correction, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.adam_w_mode = 1 if adam_w_mode else 0
        self.set_grad_none = set_grad_none
        self.capturable = bool(capturable)
        self._amp = {}  # group index -> (skipped-step counter i32[1], bias corrections f32[2]) on the device
        self._lr_dev = {}  # capturable: group index -> [device f32[1], the host value it holds]
        self._l2_slices = {}  # id(parameter) -> (weak reference to the parameter, count, coefficient): see set_l2_slice

    def set_l2_slice(self, param: torch.Tensor, count: int, coeff: float):
        """The step adds coeff * p to the gradient of the first `count` elements of `param` (not in apex).  A loss term lambda * mean(w^2) over
        such a slice has exactly this gradient with coeff = 2 lambda / n, also under a GradScaler (scaled with the loss, unscaled in the
        step); taking it here spares autograd a dense gradient of the whole parameter for a few thousand weights.  count = 0 removes it.
        EXCLUSIVE with the loss-term form: whoever installs a slice must drop the term from the loss (and remove the slice again before going
        back to a loss that contains it, `clear_l2_slices()`), or the decay is applied twice.  The entry is tied to the parameter OBJECT (weak
        reference): a tensor that replaces the parameter never inherits it, even if it reuses the id.
        Returns the installed entry as a token: `remove_l2_slice(param, token)` removes the slice only while that very entry is still the
        installed one, so an owner that goes away late (a GraphedIteration dropped after its successor was built on the same optimizer)
        cannot take its successor's slice with it."""
        if count <= 0:
            self._l2_slices.pop(id(param), None)
            return None
        entry = (weakref.ref(param), int(count), float(coeff))
        self._l2_slices[id(param)] = entry
        return entry

    def remove_l2_slice(self, param: torch.Tensor, token=None) -> bool:
        """Remove the slice of `param`; with a token (what set_l2_slice returned) only if that entry is still the installed one."""
        entry = self._l2_slices.get(id(param))
        if entry is None or (token is not None and entry is not token):
            return False
        del self._l2_slices[id(param)]
        return True

    def clear_l2_slices(self) -> None:
        """Remove every slice, whoever installed it (going back to a loss that contains the term)."""
        self._l2_slices.clear()

    def _l2_slice_of(self, p) -> tuple[int, float]:
        entry = self._l2_slices.get(id(p))
        if entry is None:
            return 0, 0.0
        if entry[0]() is not p:   # the parameter the slice was installed for is gone and its id was reused
            del self._l2_slices[id(p)]
            return 0, 0.0
        return entry[1], entry[2]

    def effective_step(self, group) -> int:
        """Step count that entered the bias corrections: group['step'] minus the overflow-skipped steps (host read, for tests / logging)."""
        if torch.is_tensor(group.get('step')):
            return int(group['step'].item())
        # by identity: list.index compares the group dicts with ==, which truth-tests tensor == tensor on their 'params' lists
        gi = next((i for i, g in enumerate(self.param_groups) if g is group), None)
        entry = self._amp.get(gi)
        return group.get('step', 0) - (int(entry[0].item()) if entry is not None else 0)

    def sync_hyperparameters(self) -> None:
        """capturable mode: write every group's current 'lr' to the device scalar the (possibly recorded) kernels read."""
        for gi, group in enumerate(self.param_groups):
            slot = self._lr_dev.get(gi)
            if slot is not None and slot[1] != float(group['lr']):
                slot[0].fill_(float(group['lr']))
                slot[1] = float(group['lr'])

    def _device_scalars(self, gi, group, device):
        """(bias corrections f32[2], skipped-step counter, device step or None, device lr or None) of a group."""
        entry = self._amp.get(gi)
        if entry is None or entry[0].device != device:
            entry = self._amp[gi] = (torch.zeros(1, dtype=torch.int32, device=device), torch.ones(2, dtype=torch.float32, device=device))
        if not self.capturable:
            return entry[1], entry[0], None, None
        if not torch.is_tensor(group.get('step')):
            group['step'] = torch.full((1,), int(group.get('step', 0)), dtype=torch.int32, device=device)
        slot = self._lr_dev.get(gi)
        if slot is None or slot[0].device != device:
            slot = self._lr_dev[gi] = [torch.full((1,), float(group['lr']), dtype=torch.float32, device=device), float(group['lr'])]
        elif slot[1] != float(group['lr']) and not torch.cuda.is_current_stream_capturing():
            slot[0].fill_(float(group['lr']))
            slot[1] = float(group['lr'])
        return entry[1], entry[0], group['step'], slot[0]

    def state_dict(self):
        """torch's layout plus, per group, 'skipped_steps': the overflow-skipped steps that nrc_adam_prepare subtracts from group['step'] for the
        bias corrections (a device counter; without it a resumed AMP run would forget its skips).  One host read per group, at save time only.
        Capturable mode saves the EFFECTIVE step (the device counter only advances on steps that were taken) with skipped_steps = 0."""
        sd = super().state_dict()
        for gi, g in enumerate(sd['param_groups']):
            entry = self._amp.get(gi)
            if torch.is_tensor(g.get('step')):
                g['step'] = int(g['step'].item())
                g['skipped_steps'] = 0
            else:
                g['skipped_steps'] = int(entry[0].item()) if entry is not None else 0
        return sd

    def load_state_dict(self, state_dict):
        """The device scalars a recorded iteration holds raw pointers to (skipped counter, bias corrections, learning rate, capturable step)
        keep their storage: they are UPDATED IN PLACE, never replaced (a replay after a load would otherwise read and write blocks that went
        back to the allocator).  A checkpoint from the non-capturable mode (step = host count incl. skips, skipped_steps = k) loaded into a
        capturable optimizer becomes device step = step - k, the count the bias corrections follow in that mode."""
        live_steps = {gi: g['step'] for gi, g in enumerate(self.param_groups) if torch.is_tensor(g.get('step'))}
        # the moment tensors too: torch's load replaces them with new storage, but a recorded iteration (nerficg_amd.graphs) holds raw pointers to
        # the LIVE exp_avg / exp_avg_sq -- the loaded values are copied into those and the live tensors go back into the state (advisor finding, round 4)
        live_moments = {id(p): (st['exp_avg'], st['exp_avg_sq']) for p, st in self.state.items() if 'exp_avg' in st and 'exp_avg_sq' in st}
        super().load_state_dict(state_dict)
        for p, st in self.state.items():
            kept = live_moments.get(id(p))
            if kept is None or 'exp_avg' not in st:
                continue
            for name, live in zip(('exp_avg', 'exp_avg_sq'), kept):
                loaded = st[name]
                if loaded is not live and loaded.shape == live.shape and loaded.dtype == live.dtype and loaded.device == live.device:
                    live.copy_(loaded)
                    st[name] = live
        self.__dict__.pop('_fused_mirror', None)      # (the fused scaler step re-derives its device step counter from the loaded counts)
        for gi, group in enumerate(self.param_groups):
            skipped = int(group.pop('skipped_steps', 0))
            step = group.get('step', 0)
            step = int(step.item()) if torch.is_tensor(step) else int(step)
            entry = self._amp.get(gi)
            if self.capturable:
                step, skipped = step - skipped, 0      # the device step counts taken steps only
                dev_step = live_steps.get(gi)
                if dev_step is not None:
                    dev_step.fill_(step)
                    group['step'] = dev_step
                else:
                    group['step'] = step               # becomes a device tensor on the first step()
            else:
                group['step'] = step
            if entry is not None:
                entry[0].fill_(skipped)
            elif skipped:
                device = group['params'][0].device
                self._amp[gi] = (torch.full((1,), skipped, dtype=torch.int32, device=device), torch.ones(2, dtype=torch.float32, device=device))
            slot = self._lr_dev.get(gi)
            if slot is not None:
                slot[0].fill_(float(group['lr']))
                slot[1] = float(group['lr'])

    def _amp_fused_step(self, scale: torch.Tensor, growth_tracker: torch.Tensor, growth_factor: float, backoff_factor: float, growth_interval: int) -> bool:
        """GradScaler.step + this step + GradScaler.update as ONE library call / two launches (nrc_amp_adam_step): inf / NaN check of the gradients
        whose last workgroup settles the step counter, the bias corrections and the scaler's scale rule, then Adam on the (one or two) parameter
        vectors.  For nerficg_amd.amp.GradScaler, which calls it when the optimizer has ONE group of at most two contiguous f32 device vectors with
        gradients (InstantNGP: Trainer.py:35) and returns False otherwise (the caller then takes the general path).  Same arithmetic as step()."""
        if len(self.param_groups) != 1:
            return False
        group = self.param_groups[0]
        params = [p for p in group['params'] if p.grad is not None]
        if not 1 <= len(params) <= 2 or not group['bias_correction']:
            return False
        dev = params[0].device
        if scale.device != dev or any(p.device != dev or p.dtype != torch.float32 or p.grad.dtype != torch.float32 or p.grad.is_sparse or not p.is_contiguous()
                                      or not p.grad.is_contiguous() for p in params):
            return False
        lib = _lib.load()
        beta1, beta2 = group['betas']
        bc_dev, skipped, step_dev, lr_dev = self._device_scalars(0, group, dev)
        if not self.capturable:
            # the host counts every call (apex), the kernel counts the steps that were taken: a device counter = host count - skipped steps rides
            # along; it is (re)derived with one host read whenever something else has moved the host count since the last fused step
            if torch.is_tensor(group.get('step')):
                group['step'] = int(group['step'].item())
            mirror = self.__dict__.setdefault('_fused_mirror', {})
            slot = mirror.get(0)
            if slot is None or slot[1] != group.get('step', 0) or slot[0].device != dev:
                slot = mirror[0] = [torch.full((1,), int(group.get('step', 0)) - int(skipped.item()), dtype=torch.int32, device=dev), group.get('step', 0)]
            step_dev = slot[0]
            group['step'] = slot[1] = group.get('step', 0) + 1
        aux = self.__dict__.setdefault('_fused_aux', {})
        if aux.get('dev') != dev:
            aux.update(dev=dev, state=torch.zeros(4, dtype=torch.float32, device=dev), ticket=torch.zeros(17 * 16, dtype=torch.int32, device=dev))
        args = []
        owners = []
        for p in params:
            state = self.state[p]
            if len(state) == 0:
                state['exp_avg'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            owner = getattr(p, '_nrc_half_owner', None)
            owner = owner() if owner is not None else None
            half = owner._half_for_optimizer(p) if owner is not None else None
            l2 = self._l2_slice_of(p)
            args += [_lib.ptr(p), _lib.ptr(p.grad), _lib.ptr(state['exp_avg']), _lib.ptr(state['exp_avg_sq']), _lib.ptr(half), p.numel(), l2[1], l2[0]]
            owners.append(owner)
        if len(params) == 1:
            args += [None, None, None, None, None, 0, 0.0, 0]
        _lib.check(lib.nrc_amp_adam_step(*args, float(group['lr']), _lib.ptr(lr_dev), float(beta1), float(beta2), float(group['eps']), float(group['weight_decay']),
                                         self.adam_w_mode, _lib.ptr(step_dev), _lib.ptr(bc_dev), _lib.ptr(scale), _lib.ptr(growth_tracker), float(growth_factor),
                                         float(backoff_factor), int(growth_interval), _lib.ptr(aux['state']), _lib.ptr(aux['ticket']),
                                         None if self.capturable else _lib.ptr(skipped), _lib.stream_of(params[0])), 'amp_adam_step')
        for p, owner in zip(params, owners):
            torch.autograd.graph.increment_version(p)
            if owner is not None:
                owner._half_written_by_optimizer(p)
        return True

    def _step_multi(self, lib) -> bool:
        """The plain step over several groups as ONE launch (nrc_adam_step_multi: apex's multi-tensor apply; the 3DGS model's six single-tensor groups with
        their own learning rates, Model.py:121-138).  False (nothing done) when a group needs something the multi-tensor kernel does not carry -- other
        betas / eps / weight decay than the first group, an L2 slice, an fp16 compute copy, non-f32 or non-contiguous tensors, more than 12 tensors."""
        first = self.param_groups[0]
        todo = []
        for group in self.param_groups:
            if (group['betas'] != first['betas'] or group['eps'] != first['eps'] or group['weight_decay'] != first['weight_decay']
                    or torch.is_tensor(group.get('step'))):
                return False
            for p in group['params']:
                if p.grad is None:
                    continue
                if (p.grad.is_sparse or p.dtype != torch.float32 or p.grad.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous()
                        or not p.grad.is_contiguous() or getattr(p, '_nrc_half_owner', None) is not None or self._l2_slice_of(p)[0]):
                    return False
                todo.append((group, p))
        if not 1 < len(todo) <= 12 or len({p.device for _, p in todo}) != 1:
            return False
        stepped = set()
        rows = []
        for group, p in todo:
            if id(group) not in stepped:       # like apex: one step counter per group, advanced whenever the group has gradients
                group['step'] = group.get('step', 0) + 1
                stepped.add(id(group))
            state = self.state[p]
            if len(state) == 0:
                state['exp_avg'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            beta1, beta2 = group['betas']
            bc = (1.0 - beta1 ** group['step'], 1.0 - beta2 ** group['step']) if group['bias_correction'] else (1.0, 1.0)
            rows.append((p, p.grad, state['exp_avg'], state['exp_avg_sq'], float(group['lr']), bc))
        n = len(rows)
        ptrs = lambda k: ctypes.cast((ctypes.c_void_p * n)(*[r[k].data_ptr() for r in rows]), ctypes.c_void_p)
        sizes = (ctypes.c_int64 * n)(*[r[0].numel() for r in rows])
        lrs = (ctypes.c_float * n)(*[r[4] for r in rows])
        bc1 = (ctypes.c_float * n)(*[r[5][0] for r in rows])
        bc2 = (ctypes.c_float * n)(*[r[5][1] for r in rows])
        cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
        beta1, beta2 = first['betas']
        _lib.check(lib.nrc_adam_step_multi(n, ptrs(0), ptrs(1), ptrs(2), ptrs(3), cast(sizes), cast(lrs), cast(bc1), cast(bc2), float(beta1), float(beta2),
                                           float(first['eps']), float(first['weight_decay']), self.adam_w_mode, _lib.stream_of(rows[0][0])), 'adam_step_multi')
        for r in rows:
            torch.autograd.graph.increment_version(r[0])
        return True

    def _step_rows(self, visibility) -> None:
        """step(visibility=...): the visibility-masked step (nrc_adam_step_rows_multi, include/nerficg_hip.h group 24).  Every check runs before any state is
        created, any counter advanced or any launch made; the counters and bias corrections are those of _step_multi (one per group, global count)."""
        todo = [(group, p) for group in self.param_groups for p in group['params'] if p.grad is not None]
        if not todo:       # e.g. right after densify_and_prune: fresh parameters, and a mask of the old length -- skipped silently like the dense step
            return
        if not torch.is_tensor(visibility):
            raise ValueError(f'FusedAdam.step: visibility must be a tensor of shape (P,), got {type(visibility).__name__}')
        if visibility.dtype not in (torch.bool, torch.uint8, torch.int32):
            raise ValueError(f'FusedAdam.step: visibility must have dtype torch.bool, torch.uint8 or torch.int32 (the rasterizer\'s radii), got {visibility.dtype}')
        if visibility.dim() != 1 or not visibility.is_contiguous():
            raise ValueError(f'FusedAdam.step: visibility must be a contiguous tensor of shape (P,), got shape {tuple(visibility.shape)}')
        if self.capturable:
            raise RuntimeError('FusedAdam.step: visibility= is not implemented for a capturable optimizer (the masked step takes host step counts)')
        if getattr(self, 'grad_scale', None) is not None or getattr(self, 'found_inf', None) is not None:
            raise RuntimeError('FusedAdam.step: visibility= together with a GradScaler (grad_scale / found_inf are set) is not implemented')
        P = visibility.shape[0]
        names = {id(p): f"parameter {k} of group {gi} ({group.get('name', 'unnamed')})"
                 for gi, group in enumerate(self.param_groups) for k, p in enumerate(group['params'])}
        for group, p in todo:
            who = names[id(p)]
            if not p.is_cuda or p.device != visibility.device:
                raise RuntimeError(f'FusedAdam.step(visibility=): {who} must be a CUDA tensor on the device of visibility ({p.device} / {visibility.device})')
            if p.grad.is_sparse or p.grad.layout != torch.strided:
                raise RuntimeError(f'FusedAdam.step(visibility=): {who} has a sparse gradient; a dense float32 gradient is needed')
            if p.dtype != torch.float32 or p.grad.dtype != torch.float32:
                raise RuntimeError(f'FusedAdam.step(visibility=): {who} and its gradient must be float32, got {p.dtype} / {p.grad.dtype}')
            if not p.is_contiguous() or not p.grad.is_contiguous():
                raise RuntimeError(f'FusedAdam.step(visibility=): {who} and its gradient must be contiguous')
            if p.dim() < 1 or p.shape[0] != P:
                raise ValueError(f'FusedAdam.step(visibility=): {who} has shape {tuple(p.shape)}, visibility has {P} rows')
            if getattr(p, '_nrc_half_owner', None) is not None:
                raise RuntimeError(f'FusedAdam.step(visibility=): {who} has an fp16 compute copy, which the masked step does not write')
            if self._l2_slice_of(p)[0]:
                raise RuntimeError(f'FusedAdam.step(visibility=): {who} has an L2 slice, which the masked step does not carry')
            state = self.state.get(p)
            if state:
                for name in ('exp_avg', 'exp_avg_sq'):
                    t = state.get(name)
                    if (not torch.is_tensor(t) or t.dtype != torch.float32 or t.device != p.device or not t.is_contiguous() or t.shape != p.shape):
                        raise RuntimeError(f'FusedAdam.step(visibility=): {name} of {who} must be a contiguous float32 tensor of the parameter\'s shape and device')
        lib = _lib.load()
        stepped = set()
        batches: dict = {}       # (betas, eps, weight_decay) -> rows, in the order of first appearance
        for group, p in todo:
            if id(group) not in stepped:       # like apex: one step counter per group, advanced whenever the group has gradients
                if torch.is_tensor(group.get('step')):   # the group was stepped in capturable mode before
                    group['step'] = int(group['step'].item())
                group['step'] = group.get('step', 0) + 1
                stepped.add(id(group))
            state = self.state[p]
            if len(state) == 0:
                state['exp_avg'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            beta1, beta2 = group['betas']
            bc = (1.0 - beta1 ** group['step'], 1.0 - beta2 ** group['step']) if group['bias_correction'] else (1.0, 1.0)
            key = (float(beta1), float(beta2), float(group['eps']), float(group['weight_decay']))
            if p.numel() > 0:
                batches.setdefault(key, []).append((p, p.grad, state['exp_avg'], state['exp_avg_sq'], float(group['lr']), bc))
        kind = 1 if visibility.dtype == torch.int32 else 0
        cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
        for (beta1, beta2, eps, weight_decay), all_rows in batches.items():
            for start in range(0, len(all_rows), 12):
                rows = all_rows[start:start + 12]
                n = len(rows)
                ptrs = lambda k: cast((ctypes.c_void_p * n)(*[r[k].data_ptr() for r in rows]))
                widths = (ctypes.c_int32 * n)(*[r[0].numel() // P for r in rows])
                lrs = (ctypes.c_float * n)(*[r[4] for r in rows])
                bc1 = (ctypes.c_float * n)(*[r[5][0] for r in rows])
                bc2 = (ctypes.c_float * n)(*[r[5][1] for r in rows])
                _lib.check(lib.nrc_adam_step_rows_multi(n, ptrs(0), ptrs(1), ptrs(2), ptrs(3), cast(widths), P, _lib.ptr(visibility), kind, cast(lrs), cast(bc1),
                                                        cast(bc2), beta1, beta2, eps, weight_decay, self.adam_w_mode, _lib.stream_of(rows[0][0])),
                           'adam_step_rows_multi')
        for _, p in todo:
            torch.autograd.graph.increment_version(p)

    def zero_grad(self, set_to_none: bool | None = None):
        super().zero_grad(set_to_none=self.set_grad_none if set_to_none is None else set_to_none)

    @torch.no_grad()
    def step(self, closure=None, *, visibility=None):
        """visibility (keyword only, default None: the dense step): a (P,) tensor on the parameters' device, torch.bool / torch.uint8 (non-zero = visible) or
        torch.int32 (the rasterizer's radii as they are, > 0 = visible).  Rows of every parameter (all of shape (P, ...)) that the mask calls invisible keep
        their values and both moments bit for bit, whatever their gradient holds; every other row gets the ordinary update, weight decay included.  The step
        counters and bias corrections stay global (one per group, as in the dense step): no per-row step count is kept.  Not with `capturable`, a GradScaler,
        an fp16 compute copy or an L2 slice; every parameter with a gradient must be contiguous float32 on the device (RuntimeError / ValueError before
        anything is modified).  A call in which no parameter has a gradient returns at once, whatever the mask."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if visibility is not None:
            self._step_rows(visibility)
            return loss
        lib = _lib.load()
        grad_scale = getattr(self, 'grad_scale', None)
        found_inf = getattr(self, 'found_inf', None)
        if not self.capturable and grad_scale is None and found_inf is None and len(self.param_groups) > 1 and self._step_multi(lib):
            return loss
        for gi, group in enumerate(self.param_groups):
            if not any(p.grad is not None for p in group['params']):
                continue
            beta1, beta2 = group['betas']
            bc1 = bc2 = 1.0
            bc_dev = lr_dev = None
            if self.capturable:
                device = next(p.device for p in group['params'] if p.grad is not None)
                bc_dev, skipped, step_dev, lr_dev = self._device_scalars(gi, group, device)
                _lib.check(lib.nrc_adam_prepare(0, float(beta1), float(beta2), _lib.ptr(found_inf), _lib.ptr(skipped), _lib.ptr(step_dev),
                                                _lib.ptr(bc_dev), _lib.stream_of(bc_dev)), 'adam_prepare')
                if not group['bias_correction']:
                    bc_dev = None
            else:
                # like apex: one step counter per group, advanced whenever the group has gradients
                if torch.is_tensor(group.get('step')):  # the group was stepped in capturable mode before
                    group['step'] = int(group['step'].item())
                group['step'] = group.get('step', 0) + 1
                if group['bias_correction']:
                    bc1, bc2 = 1.0 - beta1 ** group['step'], 1.0 - beta2 ** group['step']
                    if found_inf is not None:
                        bc_dev, skipped, _, _ = self._device_scalars(gi, group, found_inf.device)
                        _lib.check(lib.nrc_adam_prepare(int(group['step']), float(beta1), float(beta2), _lib.ptr(found_inf), _lib.ptr(skipped), None,
                                                        _lib.ptr(bc_dev), _lib.stream_of(found_inf)), 'adam_prepare')
            for p in group['params']:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError('FusedAdam does not support sparse gradients, please consider SparseAdam instead')
                if p.dtype != torch.float32 or p.grad.dtype != torch.float32:
                    raise RuntimeError('nerficg_amd FusedAdam: only float32 parameters / gradients are implemented')
                state = self.state[p]
                if len(state) == 0:
                    state['exp_avg'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                for t, name in ((p, 'param'), (state['exp_avg'], 'exp_avg'), (state['exp_avg_sq'], 'exp_avg_sq')):
                    _lib.check_input(t, name, torch.float32)
                owner = getattr(p, '_nrc_half_owner', None)
                owner = owner() if owner is not None else None
                half = owner._half_for_optimizer(p) if owner is not None else None
                l2 = self._l2_slice_of(p)
                _lib.check(lib.nrc_adam_step(
                    _lib.ptr(p), _lib.ptr(g), _lib.ptr(state['exp_avg']), _lib.ptr(state['exp_avg_sq']), p.numel(), float(group['lr']), float(beta1),
                    float(beta2), float(group['eps']), float(group['weight_decay']), self.adam_w_mode, float(bc1), float(bc2), _lib.ptr(bc_dev),
                    _lib.ptr(lr_dev), _lib.ptr(grad_scale), _lib.ptr(found_inf), _lib.ptr(half), l2[1], l2[0], _lib.stream_of(p)), 'adam_step')
                # the kernel writes through a raw pointer: tell autograd (and every version-keyed cache) that p changed
                torch.autograd.graph.increment_version(p)
                if owner is not None:
                    owner._half_written_by_optimizer(p)
        return loss
