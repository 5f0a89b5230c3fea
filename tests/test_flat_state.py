"""flat.FlatAdam on CPU tensors: one network's parameters, gradients and Adam
moments as flat buffers the module and a torch Adam see as views.  No native
library, no GPU."""
import pytest
import torch
import torch.nn as nn

from adversarial_learning_on_pointclouds_amd.flat import FlatAdam, set_optimizer_step

OFFSETS = [0, 64, 128, 192]  # Linear(5,7): 35 + 7 floats, Linear(7,3): 21 + 3, each padded to 64


def _net(seed=0):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(5, 7), nn.ReLU(), nn.Linear(7, 3))


def _steps(model, opt, n, first=0):
    for k in range(first, first + n):
        torch.manual_seed(100 + k)
        x = torch.randn(4, 5)
        opt.zero_grad(set_to_none=False)
        model(x).square().sum().backward()
        opt.step()


def _trained(n=3):
    model = _net()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    _steps(model, opt, n)
    return model, opt


def _base(t, flat, off):
    return t.data_ptr() == flat.data_ptr() + 4 * off


def test_sequential_layout_values_and_views():
    model, opt = _trained()
    before = [p.detach().clone() for p in model.parameters()]
    moments = [(opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone())
               for p in model.parameters()]
    f = FlatAdam(model, opt, "cpu")
    assert f.offsets == OFFSETS and f.numel == 256
    assert [f.layout[n] for n, _ in model.named_parameters()] == OFFSETS
    assert f.t0 == 3
    for p, b, (m, v), gv, o in zip(model.parameters(), before, moments, f.grad_views, OFFSETS):
        assert torch.equal(p.detach(), b)
        assert _base(p.data, f.param, o) and _base(p.grad, f.grad, o) and p.grad is gv
        st = opt.state[p]
        assert _base(st["exp_avg"], f.m, o) and _base(st["exp_avg_sq"], f.v, o)
        assert torch.equal(st["exp_avg"], m) and torch.equal(st["exp_avg_sq"], v)
        assert float(st["step"]) == 3.0 and st["step"].device.type == "cpu"
    views = f.views(f.m)
    assert list(views) == [n for n, _ in model.named_parameters()]
    assert all(_base(views[n], f.m, o) for n, o in zip(views, OFFSETS))


def test_bound_step_equals_untouched_twin():
    model, opt = _trained()
    twin, opt_twin = _trained()
    f = FlatAdam(model, opt, "cpu")
    old = [t.clone() for t in (f.param, f.m, f.v)]
    _steps(model, opt, 1, first=3)       # writes f.grad through the views, then Adam in place
    _steps(twin, opt_twin, 1, first=3)
    assert all(not torch.equal(t, o) for t, o in zip((f.param, f.m, f.v), old))
    for p, q, o in zip(model.parameters(), twin.parameters(), OFFSETS):
        assert _base(p.data, f.param, o) and torch.equal(p.detach(), q.detach())
        assert torch.equal(opt.state[p]["exp_avg"], opt_twin.state[q]["exp_avg"])
        assert torch.equal(opt.state[p]["exp_avg_sq"], opt_twin.state[q]["exp_avg_sq"])
        assert float(opt.state[p]["step"]) == 4.0


def test_explicit_layout_with_gap_and_mismatch():
    model = _net()
    names = [n for n, _ in model.named_parameters()]
    layout = dict(zip(names, [0, 100, 300, 40]))
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    f = FlatAdam(model, None, "cpu", layout, 400)
    assert f.numel == 400 and f.offsets == [0, 100, 300, 40]
    for n, p in model.named_parameters():
        assert _base(p.data, f.param, layout[n]) and torch.equal(p.detach(), before[n])
        assert torch.equal(f.param[layout[n]:layout[n] + p.numel()], before[n].reshape(-1))
    assert float(f.param[35:40].abs().sum()) == 0.0  # the gap stays zero
    assert FlatAdam(_net(), None, "cpu", layout).numel == 321  # the furthest tensor's end
    bad = dict(layout)
    bad["3.weight"] = bad.pop("2.weight")
    with pytest.raises(ValueError, match="do not match the fused-step layout"):
        FlatAdam(_net(), None, "cpu", bad, 400)


def test_shared_gradient_buffer():
    a, b = _net(1), _net(2)
    grad = torch.zeros(512)
    fa = FlatAdam(a, None, "cpu", grad=grad[:256])
    fb = FlatAdam(b, None, "cpu", grad=grad[256:])
    for f, mod, base in ((fa, a, 0), (fb, b, 256)):
        assert f.grad.data_ptr() == grad.data_ptr() + 4 * base
        for p, o in zip(mod.parameters(), OFFSETS):
            assert _base(p.grad, grad, base + o)
    with pytest.raises(ValueError):
        FlatAdam(_net(3), None, "cpu", grad=grad[:200])


def test_without_optimizer_binds_data_and_grad_only():
    model = _net()
    f = FlatAdam(model, None, "cpu")
    assert f.t0 == 0 and f.optimizer is None
    assert float(f.m.abs().sum()) == 0.0 and float(f.v.abs().sum()) == 0.0
    for p, o in zip(model.parameters(), OFFSETS):
        assert _base(p.data, f.param, o) and _base(p.grad, f.grad, o)


def test_state_dict_round_trip():
    model, opt = _trained()
    f = FlatAdam(model, opt, "cpu")
    fresh = torch.optim.Adam(model.parameters(), lr=1e-2)
    fresh.load_state_dict(opt.state_dict())
    g = FlatAdam(model, fresh, "cpu")
    assert g.t0 == 3 and torch.equal(g.m, f.m) and torch.equal(g.v, f.v)
    assert torch.equal(g.param, f.param) and g.m.data_ptr() != f.m.data_ptr()


def test_set_optimizer_step_plain_group_is_a_cpu_scalar():
    model, opt = _trained()
    FlatAdam(model, opt, "cpu")
    set_optimizer_step(opt, 11)
    for p in model.parameters():
        s = opt.state[p]["step"]
        assert s.device.type == "cpu" and s.dtype == torch.float32 and s.dim() == 0
        assert float(s) == 11.0
    set_optimizer_step(None, 5)  # a network without an optimizer: nothing to do
