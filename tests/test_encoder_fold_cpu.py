"""The Encoder's folded forward on the torch path (CPU, fp64): with GEOT_ENCODER_FOLD on, off, and in the reference op
order the outputs, every parameter gradient and the running statistics agree to fp64 rounding -- the composite weight
(W_f W1b) r = W_f (W1b r) and the segment addend reorder sums and nothing more.  (On the CPU thin_bn_act and
bn_act(seg=) take their torch compositions: this checks the wiring, the kernels have tests/test_encoder_fold_gpu.py.)"""
import pytest
import torch


@pytest.mark.parametrize("bs,g,n", [(2, 3, 32), (1, 1, 4), (2, 2, 6)])
def test_encoder_fold_fp64_cpu(bs, g, n, monkeypatch):
    from geot_amd.openpoints.models.backbone.transformer import Encoder
    gen = torch.Generator().manual_seed(bs * 10 + n)
    pts = torch.randn(bs, g, n, 3, generator=gen, dtype=torch.float64)
    up = torch.randn(bs, g, 32, generator=gen, dtype=torch.float64)
    torch.manual_seed(0)
    base = Encoder(32, factored=False).double().train()
    res = {}
    for name, factored, env in (("fold", True, "1"), ("unfolded", True, "0"), ("reference", False, "1")):
        monkeypatch.setenv("GEOT_ENCODER_FOLD", env)
        enc = Encoder(32, factored=factored).double().train()
        enc.load_state_dict(base.state_dict())
        out = enc(pts)
        (out * up).sum().backward()
        res[name] = (out.detach(), {k: p.grad.detach() for k, p in enc.named_parameters()},
                     {k: b.detach().clone() for k, b in enc.named_buffers()})
    for other in ("unfolded", "reference"):
        a, b = res[other][0], res["fold"][0]
        assert float((a - b).abs().max()) <= 1e-10 * float(a.abs().max()), other
        assert set(res[other][1]) == set(res["fold"][1])
        for k, ga in res[other][1].items():
            gb = res["fold"][1][k]
            # (the biases in front of a BatchNorm have a zero gradient: the scale is their weight's there)
            scale = float(res[other][1][k[:-4] + "weight"].abs().max()) if k.endswith("bias") else float(ga.abs().max())
            assert float((ga - gb).abs().max()) <= 1e-9 * scale + 1e-300, (other, k, float((ga - gb).abs().max()), scale)
        for k, ba in res[other][2].items():
            bb = res["fold"][2][k].double()
            assert float((ba.double() - bb).abs().max()) <= 1e-10 * (float(ba.double().abs().max()) + 1e-300), (other, k)
