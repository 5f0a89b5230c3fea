"""The dual discriminator on the CPU: the float64 restatement (dualdisc_ref.py)
against the reference's own float64 run (fixture g18's d64.* entries, the
reference's loop on recorded predictions), the three torch modules against the
fixture, and the eager D part of the training loop."""
import types

import numpy as np
import pytest
import torch

import dualdisc_ref as R
from dualdisc_cases import (LEFT_OUT, assert_fx_close, assert_param_close, POINT_NCLS, POINT_ROWS, dual_specs, g18_params, point_case,
                            point_last_layer, point_seed, top2_gap_share)
from golden_util import load, rel_err


@pytest.fixture(scope="module")
def fx():
    return load("g18_segdual_step.npz")


def run_restatement(fx, **quirks):
    """Two iterations of the restated D side on the fixture's recorded
    predictions.  Returns the per-iteration results and states."""
    p = g18_params(fx)
    st = R.new_state(p["S"], p["H"], p["P"])
    res = []
    for i in range(int(fx["iters"])):
        r = R.d_iteration(st, fx[f"it{i}.pred_gt"], fx[f"it{i}.pred_ng"], fx[f"it{i}.cls_gt"],
                          fx[f"it{i}.soft_gt"], fx[f"it{i}.soft_ng"], float(fx["lr_D_point"]),
                          float(fx["lr_D_shape"]), float(fx["lambda_disc_shape"]), **quirks)
        r["upd"] = {k: {n: st[k][n] - p[k][n].astype(np.float64) for n in st[k]}
                    for k in ("S", "H", "P")}
        res.append(r)
    return res


def check_restatement(fx, res):
    for i, r in enumerate(res):
        M = int(fx["B"]) * int(fx["N"])
        out = r["point"]["out"]
        assert np.abs(out[:M] - fx[f"d64.it{i}.point_gt"].reshape(-1)).max() <= 1e-9
        assert np.abs(out[M:] - fx[f"d64.it{i}.point_nogt"].reshape(-1)).max() <= 1e-9
        assert np.abs(r["shape"]["logits"] - fx[f"d64.it{i}.shape_logits"]).max() <= 1e-9
        for k in ("loss_adv", "loss_D_point", "loss_D_shape"):
            assert abs(r[k] - fx["d64." + k][i]) <= 1e-9, (i, k, r[k], fx["d64." + k][i])
        for net in ("S", "H", "P"):
            for n, g in r["grads"][net].items():
                assert_fx_close(fx, f"d64.it{i}.grad{net}.{n}", g, f"it{i} grad {net}.{n}")
            for n, u in r["upd"][net].items():
                assert_fx_close(fx, f"d64.it{i}.upd{net}.{n}", u, f"it{i} update {net}.{n}")


def test_restatement_vs_reference_float64(fx):
    """The restated D side reproduces the reference's float64 run over two
    iterations: outputs and losses to 1e-9, every gradient and every parameter
    update.  It would catch the three ways of tidying the loop up: a point-head
    gradient sum cleared every iteration, a shape term on the trunk of before
    optimizer_D_point.step(), and a trunk stepped once instead of twice: each
    variant is run too and must fail this very check."""
    check_restatement(fx, run_restatement(fx))
    for quirk in ("clear_A_P", "old_trunk", "step_trunk_once"):
        with pytest.raises(AssertionError):
            check_restatement(fx, run_restatement(fx, **{quirk: True}))


def _modules(fx, dtype=torch.float32):
    import adversarial_learning_on_pointclouds_amd as pc
    N = int(fx["N"])
    nets = dict(S=pc.BaseDiscNet(N, 50, 256), H=pc.ShapeDiscNet(256, int(fx["num_shapes"])),
                P=pc.PointDiscNet(256, N))
    for k, p in g18_params(fx).items():
        nets[k].load_state_dict({n: torch.from_numpy(v.copy()) for n, v in p.items()})
        nets[k].to(dtype)
    return nets


def test_modules_state_dict_and_forward(fx):
    """State-dict keys and shapes are the reference's (the trunk's unused conv4
    included); forward on the recorded predictions gives the reference's f32
    outputs; load_models('disc_dual') returns (shared, shape, point)."""
    import adversarial_learning_on_pointclouds_amd as pc
    from adversarial_learning_on_pointclouds_amd.model_utils import load_models
    nets = _modules(fx)
    for k, net in nets.items():
        got = [f"{n}:{'x'.join(map(str, v.shape))}" for n, v in net.state_dict().items()]
        assert got == list(fx[f"keys{k}"]), (k, got)
        assert [n for n, _ in dual_specs()[k]] == list(net.state_dict())
    assert "conv4.weight" in nets["S"].state_dict()
    with torch.no_grad():
        gt = nets["P"](nets["S"](torch.softmax(torch.from_numpy(fx["it0.pred_gt"]), dim=1)))
        ng = nets["P"](nets["S"](torch.log_softmax(torch.from_numpy(fx["it0.pred_ng"]), dim=1)))
    assert gt.shape == fx["it0.point_gt"].shape
    assert rel_err(gt.numpy(), fx["it0.point_gt"]) <= 1e-5
    assert rel_err(ng.numpy(), fx["it0.point_nogt"]) <= 1e-5
    # the shape head (the fixture's shape logits are on the updated trunk): in
    # float64 against the restatement
    n64 = _modules(fx, torch.float64)
    x = torch.softmax(torch.from_numpy(fx["it0.pred_gt"]).double(), dim=1)
    with torch.no_grad():
        s = n64["H"](n64["S"](x)).numpy()
    p = g18_params(fx)
    B, C, N = fx["it0.pred_gt"].shape
    rows = x.numpy().transpose(0, 2, 1).reshape(B * N, C)
    ref = R.shape_terms(rows, B, N, p["S"], p["H"], np.zeros(B, np.int64), 1.0)
    assert np.abs(s - ref["logits"]).max() <= 1e-9
    args = types.SimpleNamespace(input_pts=64, disc_indim=50, init_disc="xavier")
    shared, shape, point = load_models("disc_dual", "cpu", args)
    assert (type(shared), type(shape), type(point)) == (pc.BaseDiscNet, pc.ShapeDiscNet,
                                                        pc.PointDiscNet)
    assert shared.conv3.out_channels == 256 and shape.fc2.out_features == 16 \
        and point.input_pts == 64 and float(shared.conv1.bias.abs().max()) == 0.0


def test_eager_d_part_vs_reference(fx):
    """The D part of _seg_dual_body on the CPU, driven by the fixture's recorded
    predictions, labels and cls for two iterations: all three nets' parameters
    after each iteration within 1e-5 (relative to the parameter's largest
    entry) of the reference's float64 run, the point head's .grad the running sum, and
    conv4 bitwise unchanged."""
    from adversarial_learning_on_pointclouds_amd import trainer
    from adversarial_learning_on_pointclouds_amd.image_pool import ImagePool
    nets = _modules(fx)
    init = g18_params(fx)
    opt_shape = torch.optim.SGD(list(nets["H"].parameters()) + list(nets["S"].parameters()),
                                lr=float(fx["lr_D_shape"]))
    opt_point = torch.optim.SGD(list(nets["P"].parameters()) + list(nets["S"].parameters()),
                                lr=float(fx["lr_D_point"]))
    args = types.SimpleNamespace(device="cpu", lambda_disc_shape=float(fx["lambda_disc_shape"]))
    conv4 = nets["S"].conv4.weight.detach().clone()
    for i in range(int(fx["iters"])):
        opt_shape.zero_grad()  # the iteration's top (utils/trainer.py:2170-2172)
        t = lambda k: torch.from_numpy(fx[f"it{i}.{k}"])  # noqa: E731
        vals = trainer._seg_dual_d_part(
            nets["S"], nets["H"], nets["P"], opt_shape, opt_point, torch.nn.BCEWithLogitsLoss(),
            torch.nn.CrossEntropyLoss(), ImagePool(0), ImagePool(0),
            torch.softmax(t("pred_gt"), dim=1), torch.log_softmax(t("pred_ng"), dim=1),
            t("cls_gt"), args, soft=(t("soft_gt"), t("soft_ng")))
        assert abs(vals[0] - fx["d64.loss_D_point"][i]) <= 1e-5 * max(1, abs(vals[0]))
        assert abs(vals[1] - fx["d64.loss_D_shape"][i]) <= 1e-5 * max(1, abs(vals[1]))
        for k, net in nets.items():
            for n, p in net.named_parameters():
                assert_param_close(fx, f"d64.it{i}.upd{k}.{n}", p.detach().numpy(), init[k][n],
                                   f"it{i} {k}.{n}")
        for n, p in nets["P"].named_parameters():
            assert_fx_close(fx, f"d64.it{i}.gradP.{n}", p.grad.numpy(), f"it{i} A_P {n}")
    assert torch.equal(conv4, nets["S"].conv4.weight) and nets["S"].conv4.weight.grad is None


def test_case_generator_leaves_few_near_ties():
    """The GPU tests' generated point cases (the same shapes and seeds): by the
    restatement alone at most 0.5 % of points have their two best channels
    closer than 1e-5, and the generator's redraw is what guarantees it."""
    for n0, n1 in POINT_ROWS:
        for c in POINT_NCLS:
            case = point_case(point_seed(n0, n1, c), n0, n1, c)
            assert top2_gap_share(point_last_layer(case, n0, c)) <= LEFT_OUT
            assert case["logits"].shape == (n0 + n1, c + 3) and np.all(case["logits"][:, c:] == 7777.0)
    y = np.zeros((200, 128))
    y[:, 0] = 1.0
    y[0, 1] = 1.0 - 1e-6  # one near-tie in 200 rows: 0.5 %
    assert top2_gap_share(y) == 0.005


def test_new_exports_are_declared_and_abi_is_11():
    """Every new entry point is in include/pcadv.h, in _lib.SIGNATURES and in the
    built library; the ABI version stays 11 (additive)."""
    import os
    from adversarial_learning_on_pointclouds_amd import _lib as L
    names = ["pcadv_dual_input", "pcadv_dual_input_bwd", "pcadv_lrelu_fwd", "pcadv_lrelu_bwd",
             "pcadv_dual_point_tail_workspace_bytes", "pcadv_dual_point_tail", "pcadv_sgd"]
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "include", "pcadv.h")).read()
    lib = L.load()
    for n in names:
        assert n + "(" in hdr and L.SIGNATURES[n] and hasattr(lib, n), n
    assert L.ABI_VERSION == 11 and lib.pcadv_abi_version() == 11
    assert "pcadv_dual_tail_args" in hdr and L.DualTailArgs._fields_[0][0] == "y"
