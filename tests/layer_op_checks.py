"""What the GPU test files of the three single-layer convolution families ask of their torch operators, and of the networks trained
through them, each written once: the operator of a case under autograd, the legs it launches, its NCHW path; the output and parameter
gradients of a network, the outputs of its norm layers and the ReLU margin of its reference.  Families and cases:
tests/layer_cases.py; the bar: tests/parity.py."""
import copy

import torch

from tests import layer_cases as lc
from tests.parity import check


def op_run(fam, op_of, name, channels_last=True, need=(True, True, True)):
    """the operator on the inputs of one case, and its backward under the case's seed gradient if anything needs one.
    op_of(c) -> (the case as the operator sees it, callable(x, w, b) -> y); need: which of x, w, b ask for a gradient
    -> (y, x, w, b) on the device, the gradients on the leaves"""
    import keypointnerf_amd.torch_ops  # noqa: F401
    c, op = op_of(fam.cases[name])
    (x, w, b, g), _, _ = lc.reference(fam, name)
    xd = x.cuda().contiguous(memory_format=torch.channels_last) if channels_last else x.cuda().contiguous()
    xd.requires_grad_(need[0] and fam.has_dx(c))
    wd = w.cuda().requires_grad_(need[1])
    bd = None if b is None else b.cuda().requires_grad_(need[2])
    y = op(xd, wd, bd)
    if y.requires_grad:
        (y * g.cuda()).sum().backward()
    return y.detach(), xd, wd, bd


def check_op_launches_only_needed_legs(monkeypatch, fam, op_of, backward_attr, names, stem_name=None, name_in_label=True):
    """ops.<backward_attr> is asked for exactly the legs whose leaves need a gradient, for each case of `names` (with a bias) and, with
    a frozen weight, for the stem; what it returns meets the bar"""
    from keypointnerf_amd import ops
    seen = []
    real = getattr(ops, backward_attr)

    def spy(*a, **kw):
        seen.append((kw["want_dx"], kw["want_dw"], kw["want_db"]))
        return real(*a, **kw)

    monkeypatch.setattr(ops, backward_attr, spy)
    for name in names:
        del seen[:]
        label = f"{name} " if name_in_label else ""
        _, r64, e_ref = lc.reference(fam, name)
        _, xd, wd, bd = op_run(fam, op_of, name, need=(True, False, False))         # a frozen layer: dX alone
        assert seen == [(True, False, False)] and wd.grad is None and bd.grad is None
        check(f"{label}x only dx", xd.grad.cpu().numpy(), r64["dx"], e_ref["dx"])
        _, xd, wd, bd = op_run(fam, op_of, name, need=(False, True, False))         # a first layer with a frozen bias: dW alone
        assert seen[1:] == [(False, True, False)] and xd.grad is None and bd.grad is None
        check(f"{label}weight only dw", wd.grad.cpu().numpy(), r64["dw"], e_ref["dw"])
        _, xd, wd, bd = op_run(fam, op_of, name, need=(False, True, True))
        assert seen[2:] == [(False, True, True)] and xd.grad is None
        check(f"{label}weight and bias db", bd.grad.cpu().numpy(), r64["db"], e_ref["db"])
        y, _, _, _ = op_run(fam, op_of, name, need=(False, False, False))           # nothing: no graph, no backward call
        assert not y.requires_grad and len(seen) == 3
    if stem_name is not None:
        del seen[:]
        _, _, wd, bd = op_run(fam, op_of, stem_name, need=(False, False, True))     # the stem with a frozen weight: db alone
        assert seen == [(False, False, True)] and wd.grad is None and bd.grad is not None


def check_op_nchw_bits(fam, op_of, names):
    """an NCHW input gives the bits of the channels_last one, y comes back channels_last and the gradient of an NCHW leaf NCHW"""
    for name in names:
        a, b = op_run(fam, op_of, name, channels_last=True), op_run(fam, op_of, name, channels_last=False)
        assert torch.equal(a[0], b[0]) and torch.equal(a[2].grad, b[2].grad)
        assert b[0].is_contiguous(memory_format=torch.channels_last)
        if fam.has_dx(op_of(fam.cases[name])[0]):
            assert torch.equal(a[1].grad, b[1].grad) and b[1].grad.is_contiguous()  # the gradient of an NCHW leaf comes back NCHW


# ---- networks trained through the operators ----
def param_grads(net, x, gs, allow_unused=False):
    """gs a tensor -> {"y": output, parameter name: gradient}; gs a list, one per output -> the outputs under "y<i>".  allow_unused: a
    parameter the outputs do not depend on has the gradient None.  x needs no gradient (the stems have none to give)"""
    ys = net(x)
    ys = list(ys) if isinstance(ys, (list, tuple)) else [ys]
    many = isinstance(gs, (list, tuple))
    params = dict(net.named_parameters())
    grads = torch.autograd.grad(ys, list(params.values()), gs if many else [gs], allow_unused=allow_unused)
    out = {f"y{i}": y.detach() for i, y in enumerate(ys)} if many else {"y": ys[0].detach()}
    out.update(dict(zip(params, grads)))
    return out


def group_norms(net):
    return {n: m for n, m in net.named_modules() if isinstance(m, torch.nn.GroupNorm)}


def norm_outputs(net, x, memory_format, norms=group_norms):
    """{norm name: its output before the ReLU behind it} of the layers norms(net) -> {name: module}"""
    pre, hooks = {}, []
    for n, m in norms(net).items():
        hooks.append(m.register_forward_hook(lambda m, i, o, n=n: pre.__setitem__(n, o.detach().clone())))
    with torch.no_grad():
        net(x.contiguous(memory_format=memory_format))
    for h in hooks:
        h.remove()
    return pre


def narrow_margin(net, x, norms, n_norms, n_values=None):
    """(smallest |norm output| of the fp64 module over the layers norms(net), largest fp32 deviation of those outputs over both memory
    formats); there are n_norms such layers with n_values outputs in all"""
    pre64 = norm_outputs(copy.deepcopy(net).double(), x.double(), torch.contiguous_format, norms)
    pre32 = [norm_outputs(copy.deepcopy(net), x, mf, norms) for mf in (torch.contiguous_format, torch.channels_last)]
    assert len(pre64) == n_norms and n_values in (None, sum(p.numel() for p in pre64.values()))
    margin = min(float(p.abs().min()) for p in pre64.values())
    return margin, max(float((r[n].double() - p).abs().max()) for r in pre32 for n, p in pre64.items())
