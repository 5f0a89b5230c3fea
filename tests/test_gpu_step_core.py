"""What the fused steps' shared core turns from a silent wrong result into an
error: a discriminator optimizer whose betas differ from the generator's is
refused at construction (one pair serves both fused Adams), and a warm-up that
raises leaves the capture's state as it was.  MI355X only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.mark.parametrize("ft", [False, True])
def test_mismatched_d_betas_refused_at_construction(ft):
    import adversarial_learning_on_pointclouds_amd as pc
    from adversarial_learning_on_pointclouds_amd.step import AdvFtTrainStep, AdvTrainStep
    m = pc.PointNetCls(k=40, feature_transform=ft).to(DEV)
    d = pc.DeepConvDiscNet(40, 1).to(DEV)
    before = [p.data_ptr() for p in m.parameters()]
    opt = torch.optim.Adam(m.parameters(), lr=1e-4, betas=(0.9, 0.999))
    opt_d = torch.optim.Adam(d.parameters(), lr=1e-4, betas=(0.5, 0.999))
    with pytest.raises(ValueError, match="applies the generator optimizer's betas / eps"):
        (AdvFtTrainStep if ft else AdvTrainStep)(m, d, 2, 128, optimizer=opt, optimizer_D=opt_d)
    assert [p.data_ptr() for p in m.parameters()] == before  # refused before anything was rebound


def test_capture_restores_state_when_the_warmup_raises():
    from adversarial_learning_on_pointclouds_amd.flat import capture_graphs
    a = torch.arange(8, device=DEV, dtype=torch.float32)
    b = torch.full((3,), 7, device=DEV, dtype=torch.int32)
    a0, b0 = a.clone(), b.clone()

    def warmup():
        a.mul_(3.0)
        b.add_(1)
        raise ValueError("warm-up failed")

    with pytest.raises(ValueError, match="warm-up failed"):
        capture_graphs(torch.device(DEV), warmup, lambda: None, [a, b])
    assert torch.equal(a, a0) and torch.equal(b, b0)
