"""What the GPU test files of the three single-layer convolution families ask of their torch operators, and of the networks trained
through them, each written once: the operator of a case under autograd, the legs it launches, its NCHW path; the output and parameter
gradients of a network, the outputs of its norm layers and the ReLU margin of its reference.  Families and cases:
tests/layer_cases.py; the bar: tests/parity.py."""
import copy

import pytest
import torch

from tests import layer_cases as lc
from tests.parity import check, nchw, nhwc


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


# ---- keypointnerf_amd.ops under the operators: one cached plan per layer shape ----
def _ops_of(fam, c):
    """(pack(w), forward(x, packed, b), backward(x, dy, packed, **want)) of keypointnerf_amd.ops for a case given as its dict"""
    from keypointnerf_amd import ops
    if "kind" not in c:
        return (ops.conv2d_pack, lambda x, p, b: ops.conv2d_forward(x, p, b, c["cout"], c["k"], c["pad"]),
                lambda x, dy, p, **kw: ops.conv2d_backward(x, dy, p, c["cin"], c["k"], c["pad"], c["bias"], **kw))
    pack, fwd, bwd = (getattr(ops, fam.prefix[len("kpn_"):] + f) for f in ("pack", "forward", "backward"))
    return (lambda w: pack(w, c["kind"]), lambda x, p, b: fwd(x, p, b, c["cout"], c["kind"]),
            lambda x, dy, p, **kw: bwd(x, dy, p, (c["N"], c["cin"], c["H"], c["W"]), c["kind"], c["bias"], **kw))


def _ops_run_twice(fam, c):
    """the packer, then two forward and two backward calls of keypointnerf_amd.ops on the inputs of a case given as its dict: the two
    pairs give equal bits -> ((misses, hits, plans) the four calls added to the plan cache, (y, dx, dw, db) of the first pair)"""
    from keypointnerf_amd import ops
    x, w, b, g = lc.inputs(fam, c)
    pack, fwd, bwd = _ops_of(fam, c)
    xd = x.cuda().contiguous() if fam.x_is_nchw(c) else x.cuda().contiguous(memory_format=torch.channels_last)
    gd, bd = g.cuda().contiguous(memory_format=torch.channels_last), (None if b is None else b.cuda())
    packed = pack(w.cuda())
    before = ops._layer_plan.cache_info()
    runs = [(fwd(xd, packed, bd),) + bwd(xd, gd, packed, want_dx=fam.has_dx(c)) for _ in range(2)]
    after = ops._layer_plan.cache_info()
    for first, second in zip(*runs):
        assert (first is None and second is None) or torch.equal(first.contiguous().view(torch.int32), second.contiguous().view(torch.int32))
    return (after.misses - before.misses, after.hits - before.hits, after.currsize - before.currsize), runs[0]


def check_ops_plan_once_per_shape(fam, L, B, names, stem_name=None):
    """for each case of `names` (and the stem): four calls of one shape build one plan and look it up three times; the same layer
    with one image more builds a second one and still gives the bits of the C-ABI driver.  The stem refuses a dx by its message"""
    from keypointnerf_amd import ops
    for name in names + ((stem_name,) if stem_name else ()):
        ops._layer_plan.cache_clear()                                   # the tests before this one have planned these shapes
        c = fam.cases[name]
        added, _ = _ops_run_twice(fam, c)
        assert added == (1, 3, 1), (name, added)
        c2 = dict(c, N=c["N"] + 1)
        added, (y, dx, dw, db) = _ops_run_twice(fam, c2)
        assert added == (1, 3, 1), (name, added)
        x, w, b, g = lc.inputs(fam, c2)
        packed = lc.pack(fam, L, B, c2, w.numpy())
        y_abi = lc.forward(fam, L, B, c2, lc.x_layout(fam, c2, x), packed, None if b is None else b.numpy())
        abi = lc.backward(fam, L, B, c2, lc.x_layout(fam, c2, x), nhwc(g), packed)
        assert torch.equal(y.cpu(), torch.from_numpy(nchw(y_abi))) and torch.equal(dw.cpu(), torch.from_numpy(abi["dw"]))
        assert (dx is None) == (not fam.has_dx(c)) and (dx is None or torch.equal(dx.cpu(), torch.from_numpy(nchw(abi["dx"]))))
        assert (db is None) == (not c["bias"]) and (db is None or torch.equal(db.cpu(), torch.from_numpy(abi["db"])))
    if stem_name:
        c = fam.cases[stem_name]
        x, w, b, g = lc.inputs(fam, c)
        pack, _, bwd = _ops_of(fam, c)
        with pytest.raises(ValueError, match=f"^{fam.prefix[len('kpn_'):-1]}: the stem has no input gradient$"):
            bwd(x.cuda().contiguous(), g.cuda().contiguous(memory_format=torch.channels_last), pack(w.cuda()), want_dx=True)


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
