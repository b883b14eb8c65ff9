"""The loss switches of the FixMatch+NTM loop, host side: ABI and prototypes of the fused criteria, the reference-executed
fixture tests/golden/criteria_ref.npz (provenance, the conditions on its inputs, and a numpy restatement of the four
formulas the kernels implement against its fp64 results), the name dispatch, the cfg checks and unused_parameters()."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import make_criteria_golden as maker  # noqa: E402
from test_ref_fixtures_gpu import close  # noqa: E402

NEW_SYMBOLS = ("geot_weighted_ce", "geot_weighted_ce_grad", "geot_weighted_ce_ws_doubles", "geot_poly1_focal_beta",
               "geot_poly1_focal_beta_grad", "geot_fixmatch_meters_finalize6", "geot_ntm_feature_loss_grad_det")
UNBRANCHED = ("MSE_Loss_U", "MultiShapeCrossEntropy", "Poly1FocalLoss_U_Cur", "Poly1FocalLoss_U_top2", "Poly1FocalLoss_U_T_v1")
SIX = ("Poly1FocalLoss", "Poly1FocalLoss_U_corr", "Weight_CELoss", "Weight_CELoss_U", "Poly1FocalLoss_U", "Poly1FocalLoss_U_T")
TH = 0.95


def inputs(golden):
    """The fixture's inputs: the small ones as stored, the two logits tensors rebuilt -- and the stored ones equal the
    rebuilt ones, so the fixture's results belong to exactly these inputs."""
    ref = golden("criteria_ref.npz")
    z = maker.draw_inputs()
    for k in ("labels", "labels_u", "conf", "conf_nan", "cw2", "cw3"):
        assert np.array_equal(ref[k], z[k], equal_nan=True), k
    return ref, z


def test_abi_and_prototypes_of_the_new_entry_points():
    from geot_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "geot_hip.h")).read()
    assert int(re.search(r"GEOT_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 17
    lib = _lib.load()
    assert lib.geot_abi_version() == _lib.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.exported_symbols(), name
        assert hasattr(lib, name), name
        proto = re.search(r"\b%s\((.*?)\);" % name, hdr, flags=re.S).group(1)
        bound = _lib.PROTOTYPES[name] if name in _lib.PROTOTYPES else _lib.PLAIN[name][0]
        assert len(proto.split(",")) == len(bound), name
    assert lib.geot_weighted_ce_ws_doubles(2, 17, 16000) == 2 * 2 * 63 and lib.geot_weighted_ce_ws_doubles(1, 1, 1) == 2
    assert lib.geot_weighted_ce_ws_doubles(3, 32, 33000) == 2 * 3 * 64            # the grid cap
    for b, c, n in ((0, 17, 8), (1, 0, 8), (1, 33, 8), (1, 17, 0)):
        assert lib.geot_weighted_ce_ws_doubles(b, c, n) == -1


def test_fixture_provenance_and_input_conditions(golden):
    ref, z = inputs(golden)
    meta = str(ref["meta"])
    assert "executed from /root/reference" in meta and "Tensor.cuda = identity" in meta
    for name in maker.NAMES:
        assert re.search(r"openpoints/loss/build.py::%s lines \d+-\d+" % name, meta), name
    assert os.path.getsize(os.path.join(HERE, "golden", "criteria_ref.npz")) < \
        os.path.getsize(os.path.join(HERE, "golden", "val_batches_ref.npz"))
    assert dict(maker.THRESHOLDS) == {"t095": TH}
    maker.check_inputs(z, (TH,))
    # ... and spelled out once more, independently of the maker's own helper
    lab, lab_u, conf = ref["labels"], ref["labels_u"], ref["conf_nan"]
    with np.errstate(invalid="ignore"):
        confident = conf >= np.float32(TH)
    total = lab.size
    assert (confident & (lab_u != 0) & (lab_u != 255)).sum() >= total / 4
    assert (~confident).sum() >= total / 10 and (confident & (lab_u == 0)).sum() >= total / 10
    assert (lab_u == 255).sum() == 1 and np.isnan(conf).sum() == 1
    sel = np.take_along_axis(z["t"], lab[:, None, :], axis=1)
    assert 0.25 <= np.abs(sel).min() and np.abs(sel).max() <= 4.0 and (sel > 0).any() and (sel < 0).any()
    assert ref["cw2"].shape[0] == 2 and ref["cw3"].shape[0] == 3
    for case in ("wce_bw2", "wce_bw3", "wceu_t095", "pu_t095", "put_t095"):
        for dn in ("f32", "f64"):
            assert ref["%s_loss_%s" % (case, dn)].shape == () and ref["%s_grad_%s" % (case, dn)].shape == z["logits"].shape
            assert np.abs(ref["%s_grad_%s" % (case, dn)]).max() > 0
    assert ref["put_t095_gradt_f64"].shape == z["t"].shape


# ---- the formulas of the kernels (include/geot_hip.h), restated in numpy fp64 ---------------------------------------------
def np_weighted_ce(x, y, cw, conf=None, thresh=0.0):
    x, w = x.astype(np.float64), cw.astype(np.float64).mean(axis=0)
    b, c, n = x.shape
    e = np.exp(x - x.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    live = np.ones((b, n), bool)
    if conf is not None:
        with np.errstate(invalid="ignore"):
            live = (conf >= np.float32(thresh)) & (y != 0) & (y != 255)
    yy = np.where(live, y, 0)
    onehot = np.arange(c)[None, :, None] == yy[:, None, :]
    wy = w[yy] * live
    loss = -(wy * np.log(np.take_along_axis(p, yy[:, None, :], axis=1)[:, 0])).sum() / (b * n)
    return loss, wy[:, None, :] / (b * n) * (p - onehot)


def np_poly1(x, pos, alpha=0.25, gamma=2.0, eps=1.0):
    """-> l, dl/dx of the Poly-1 focal term."""
    p = 1.0 / (1.0 + np.exp(-x))
    ce = np.maximum(x, 0) - x * pos + np.log1p(np.exp(-np.abs(x)))
    q = np.where(pos, 1 - p, p)
    at = np.where(pos, alpha, 1 - alpha)
    dq = np.where(pos, -1.0, 1.0) * p * (1 - p)
    l = at * ce * q ** gamma + eps * q ** (gamma + 1)
    dl = at * ((p - pos) * q ** gamma + ce * gamma * q ** (gamma - 1) * dq) + eps * (gamma + 1) * q ** gamma * dq
    return l, dl


def np_poly1_masked(x, y, conf, thresh, t=None):
    x = x.astype(np.float64)
    b, c, n = x.shape
    pos = np.arange(c)[None, :, None] == y[:, None, :]
    with np.errstate(invalid="ignore"):
        keep = (conf >= np.float32(thresh)).astype(np.float64)[:, None, :]
    l, dl = np_poly1(x, pos)
    den = c * keep.sum() + 0.001
    if t is None:
        return (l * keep).sum() / den, keep * dl / den, None
    t = t.astype(np.float64)
    cf = conf.astype(np.float64)[:, None, :]
    ty = np.take_along_axis(t, y[:, None, :], axis=1)
    beta = cf / ty
    grad_t = pos * (-cf / ty ** 2) * l.sum(axis=1, keepdims=True) * keep / den
    return (l * beta * keep).sum() / den, beta * keep * dl / den, grad_t


def test_the_issue_formulas_are_the_reference(golden):
    ref, z = inputs(golden)
    for bw in (2, 3):
        loss, grad = np_weighted_ce(z["logits"], z["labels"], z["cw%d" % bw])
        close(loss, ref["wce_bw%d_loss_f64" % bw], what="wce loss")
        close(grad, ref["wce_bw%d_grad_f64" % bw], what="wce grad")
    loss, grad = np_weighted_ce(z["logits"], z["labels_u"], z["cw2"], z["conf_nan"], TH)
    close(loss, ref["wceu_t095_loss_f64"], what="wceu loss")
    close(grad, ref["wceu_t095_grad_f64"], what="wceu grad")
    with np.errstate(invalid="ignore"):
        dead = ~((z["conf_nan"] >= np.float32(TH)) & (z["labels_u"] != 0) & (z["labels_u"] != 255))
    assert dead.any() and (ref["wceu_t095_grad_f32"].transpose(0, 2, 1)[dead] == 0).all()      # the reference's, exactly 0
    loss, grad, _ = np_poly1_masked(z["logits"], z["labels"], z["conf_nan"], TH)
    close(loss, ref["pu_t095_loss_f64"], what="pu loss")
    close(grad, ref["pu_t095_grad_f64"], what="pu grad")
    loss, grad, grad_t = np_poly1_masked(z["logits"], z["labels"], z["conf"], TH, z["t"])
    close(loss, ref["put_t095_loss_f64"], what="put loss")
    close(grad, ref["put_t095_grad_f64"], what="put grad")
    close(grad_t, ref["put_t095_gradt_f64"], what="put grad_t")
    off = np.arange(maker.C)[None, :, None] != z["labels"][:, None, :]
    assert (ref["put_t095_gradt_f32"][off] == 0).all()


def test_the_torch_composites_restate_the_reference(golden):
    """On CPU tensors every class takes its composite: the fall-back of the fused path, against the same fixture."""
    from geot_amd.openpoints.loss import Poly1FocalLoss_U, Poly1FocalLoss_U_T, Weight_CELoss, Weight_CELoss_U
    ref, z = inputs(golden)
    T = torch.from_numpy
    for dn, dt in (("f32", torch.float32), ("f64", torch.float64)):
        def run(fn, *xs):
            leaves = [T(x).to(dt).requires_grad_(True) for x in xs]
            loss = fn(*leaves)
            loss.backward()
            return [loss.detach().numpy()] + [x.grad.numpy() for x in leaves]
        lab, lab_u = T(z["labels"]), T(z["labels_u"])
        for bw in (2, 3):
            got = run(lambda x: Weight_CELoss()(x, lab, T(z["cw%d" % bw]).to(dt)), z["logits"])
            close(got[0], ref["wce_bw%d_loss_%s" % (bw, dn)])
            close(got[1], ref["wce_bw%d_grad_%s" % (bw, dn)])
        got = run(lambda x: Weight_CELoss_U()(x, lab_u, T(z["cw2"]).to(dt), T(z["conf_nan"]).to(dt), thresh=TH), z["logits"])
        assert torch.equal(lab_u, T(z["labels_u"]))               # the caller's labels are left alone
        close(got[0], ref["wceu_t095_loss_" + dn])
        close(got[1], ref["wceu_t095_grad_" + dn])
        got = run(lambda x: Poly1FocalLoss_U()(x, lab, T(z["conf_nan"]).to(dt), thresh=TH), z["logits"])
        close(got[0], ref["pu_t095_loss_" + dn])
        close(got[1], ref["pu_t095_grad_" + dn])
        got = run(lambda x, t: Poly1FocalLoss_U_T()(x, lab, T(z["conf"]).to(dt), None, t, thresh=TH), z["logits"], z["t"])
        close(got[0], ref["put_t095_loss_" + dn])
        close(got[1], ref["put_t095_grad_" + dn])
        close(got[2], ref["put_t095_gradt_" + dn])


def test_build_criterion_from_cfg_resolves_six_names_and_refuses_the_unbranched_ones():
    from geot_amd.openpoints import loss as L
    for name in SIX:
        crit = L.build_criterion_from_cfg({"NAME": name})
        assert type(crit).__name__ == name and isinstance(crit, torch.nn.Module)
    crit = L.build_criterion_from_cfg({"NAME": "Poly1FocalLoss_U_T", "epsilon": 2.0, "gamma": 3.0}, alpha=-1.0)
    assert (crit.epsilon, crit.gamma, crit.alpha) == (2.0, 3.0, -1.0)
    assert L.Poly1FocalLoss_U.forward is L.Poly1FocalLoss_U_corr.forward        # the same body under its own name
    for name in UNBRANCHED:
        with pytest.raises(NotImplementedError, match=name):
            L.build_criterion_from_cfg({"NAME": name})
    with pytest.raises(KeyError, match="NoSuchLoss"):
        L.build_criterion_from_cfg({"NAME": "NoSuchLoss"})


class _NoDevice:
    """Stands where a module would: any use of it is a failure of 'before touching a device'."""

    def __getattr__(self, name):
        raise AssertionError("the step touched its modules (%s) before refusing the cfg" % name)


def test_steps_refuse_a_bad_cfg_before_touching_a_device():
    from geot_amd.train_step import NTM_CFG, FixMatchNTMStep, SupervisedStep, build_fixmatch
    defaults = dict(criterion="Poly1FocalLoss", criterion_u="Poly1FocalLoss_U_corr", use_3d_loss=True, use_feat_loss=False,
                    feat_loss_weight=10.0, feat_k=16, feat_sigma=1.0, use_identity_loss=False, identity_loss_weight=1.0)
    assert {k: NTM_CFG[k] for k in defaults} == defaults
    nd = _NoDevice()
    for name in UNBRANCHED:
        key = "criterion" if name == "MultiShapeCrossEntropy" else "criterion_u"
        with pytest.raises(NotImplementedError, match=name):
            FixMatchNTMStep(nd, nd, nd, cfg={key: name})
        with pytest.raises(NotImplementedError, match=name):
            SupervisedStep(nd, criterion=name)
        with pytest.raises(NotImplementedError, match=name):
            build_fixmatch("cuda:0", cfg={key: name})
    with pytest.raises(ValueError, match="criterion_u"):
        FixMatchNTMStep(nd, nd, nd, cfg={"criterion_u": "Weight_CELoss"})        # a supervised criterion in the other place
    with pytest.raises(ValueError, match="criterion"):
        FixMatchNTMStep(nd, nd, nd, cfg={"criterion": "Poly1FocalLoss_U"})
    with pytest.raises(ValueError, match="criterion"):
        SupervisedStep(nd, criterion="Weight_CELoss_U")
    with pytest.raises(KeyError):
        FixMatchNTMStep(nd, nd, nd, cfg={"criterion_u": "NoSuchLoss"})
    with pytest.raises(TypeError, match="use_3d_loss"):
        FixMatchNTMStep(nd, nd, nd, cfg={"use_3d_loss": "no"})
    with pytest.raises(ValueError, match="feat_k"):
        FixMatchNTMStep(nd, nd, nd, cfg={"use_feat_loss": True, "feat_k": 0})
    # the flat gradient exchange of a replayed step: a cfg that leaves a synchronised parameter without a gradient
    with pytest.raises(RuntimeError, match="sigma"):
        build_fixmatch("cuda:0", cfg={"criterion_u": "Poly1FocalLoss_U"}, graph_sync=True)


def test_unused_parameters_per_configuration():
    from geot_amd.train_step import UNUSED_FIXMATCH, unused_parameters
    base = ("T_revision.weight", "T_linear.weight")
    assert unused_parameters() == unused_parameters({}) == base == tuple(UNUSED_FIXMATCH)
    assert unused_parameters({"criterion_u": "Poly1FocalLoss_U_T", "use_3d_loss": False}) == base
    for name in ("Poly1FocalLoss_U", "Weight_CELoss_U", {"NAME": "Weight_CELoss_U"}):
        assert unused_parameters({"criterion_u": name}) == base + ("sigma",)                          # the 3-D loss is on
        assert unused_parameters({"criterion_u": name, "use_3d_loss": False}) == base + ("sigma", "T_predictor.*")
        assert unused_parameters({"criterion_u": name, "use_3d_loss": False, "use_identity_loss": True}) == base + ("sigma",)
        assert unused_parameters({"criterion_u": name, "use_3d_loss": False, "use_feat_loss": True}) == base + ("sigma",)
