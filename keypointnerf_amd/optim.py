"""Adam for the reference's training loop with the hot-path parameters stepped by one launch.

``configure_optimizers`` of the reference returns ``torch.optim.Adam(self.model.parameters(), lr=...)`` (src/model.py:46-47).
``Adam(params, net=model, ...)`` here is that optimizer — same update, same ``state_dict`` layout, loadable into and from a
``torch.optim.Adam`` — except that the parameters of ``net``'s hot-path modules (``mlp_geo.``, ``mlp_tex.``,
``ibr_compress_gfeat.``: 44 tensors of a few hundred elements each) are updated by ``kpn_adam_step`` (csrc/param_kernels.hip)
instead of a train of small kernels, and that their ``exp_avg`` / ``exp_avg_sq`` are views into two flat buffers.  Every other
parameter (the image encoders) goes through torch's own functional Adam.  There is no CPU path for the hot parameters.
"""
import torch
from torch.optim import adam as _torch_adam

from . import ops
from .dropin import _HOT_PREFIXES
from .weights import live_parameters


class Adam(torch.optim.Optimizer):
    def __init__(self, params, net=None, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, maximize=False):
        if net is None:
            raise ValueError("keypointnerf_amd.optim.Adam needs net= (the module whose hot-path parameters it steps natively)")
        if amsgrad or maximize:
            raise NotImplementedError("keypointnerf_amd.optim.Adam implements amsgrad=False, maximize=False (the reference's optimizer)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        self._hot_ids = {id(p) for n, p in live_parameters(net).items() if n.startswith(_HOT_PREFIXES)}
        self._hot_step = {}  # id(param) -> its step count as a Python integer (mirrors state[p]["step"], which stays the record)
        self._flat = {}     # id(param) -> (flat exp_avg, flat exp_avg_sq, offset): the two buffers of the parameter's group
        # the keys of torch.optim.Adam's groups, so that a state_dict moves between the two (load_state_dict copies the saved groups)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                                      foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False))

    def _is_hot(self, p):
        return id(p) in self._hot_ids and p.dtype == torch.float32 and p.is_contiguous()

    def _flat_state(self, group, p):
        """the parameter's views into its group's flat moment buffers (allocated, zeroed, on first use)"""
        if id(p) not in self._flat:
            hot = [q for q in group["params"] if self._is_hot(q)]
            m = torch.zeros(sum(q.numel() for q in hot), dtype=torch.float32, device=p.device)
            v = torch.zeros_like(m)
            o = 0
            for q in hot:
                self._flat[id(q)] = (m, v, o)
                o += q.numel()
        m, v, o = self._flat[id(p)]
        return m[o:o + p.numel()].view(p.shape), v[o:o + p.numel()].view(p.shape)

    def _init_state(self, group, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)          # on the host, as torch.optim.Adam keeps it
            if self._is_hot(p):
                st["exp_avg"], st["exp_avg_sq"] = self._flat_state(group, p)
            else:
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._hot_step.clear()
        for group in self.param_groups:                                  # the loaded moments move into the flat buffers
            if group.get("amsgrad") or group.get("maximize"):
                raise NotImplementedError("keypointnerf_amd.optim.Adam implements amsgrad=False, maximize=False")
            for p in group["params"]:
                st = self.state.get(p)
                if st and self._is_hot(p):
                    m, v = self._flat_state(group, p)
                    m.copy_(st["exp_avg"])
                    v.copy_(st["exp_avg_sq"])
                    st["exp_avg"], st["exp_avg_sq"] = m, v
                    st["step"] = torch.as_tensor(st["step"], dtype=torch.float32).cpu()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            by_step = {}                                                 # step number -> the hot tensors that take it now
            cold = ([], [], [], [], [])
            for p in group["params"]:
                if p.grad is None:
                    continue                                             # as torch: untouched, its step not advanced
                if p.grad.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                st = self._init_state(group, p)
                if self._is_hot(p):
                    if not ops._on_gpu(p):
                        raise RuntimeError("keypointnerf_amd.optim.Adam: the hot-path parameters must live on the GPU (no CPU path)")
                    t_now = self._hot_step.get(id(p))
                    if t_now is None:
                        t_now = int(st["step"])
                    self._hot_step[id(p)] = t_now + 1
                    lists = by_step.setdefault(t_now + 1, ([], [], [], [], []))
                    for lst, t in zip(lists, (p, p.grad.contiguous(), st["exp_avg"], st["exp_avg_sq"], st["step"])):
                        lst.append(t)
                else:
                    for lst, t in zip(cold, (p, p.grad, st["exp_avg"], st["exp_avg_sq"], st["step"])):
                        lst.append(t)
            for t, (ps, gs, ms, vs, steps) in sorted(by_step.items()):
                torch._foreach_add_(steps, 1)                           # the host step counts, one call
                ops.adam_step(ps, gs, ms, vs, t, group["lr"], beta1, beta2, group["eps"], group["weight_decay"])
            if cold[0]:
                _torch_adam.adam(cold[0], cold[1], cold[2], cold[3], [], cold[4], amsgrad=False, beta1=beta1, beta2=beta2, lr=group["lr"],
                                 weight_decay=group["weight_decay"], eps=group["eps"], maximize=False, foreach=group.get("foreach"),
                                 capturable=False, differentiable=False, fused=group.get("fused"),
                                 has_complex=any(torch.is_complex(p) for p in cold[0]),
                                 decoupled_weight_decay=bool(group.get("decoupled_weight_decay", False)))
        return loss
