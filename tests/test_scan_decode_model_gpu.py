"""Whole scans decoded at full resolution from one backbone pass, model level (geot_amd/validation.py decode_scans /
validate_scans_decoded, PointTransformer_seg_T.decode_front_params / decode_tail, ScanBatcher.batch(affine=True)): the smallest
model that runs a forward pass (384 wide, everything else tiny: tests/_scan_decode_ref.py TINY) in eval mode on scans of 150 and
97 vertices, jaws 0 and 1, N = 64 samples, decoded in three chunks.
(a) for the sampled vertices q equals pos bit for bit, and the decoded logits and the forward pass's own logits both lie within
the bound of the fp64 last stage restated from the kept f_l1 (so within the summed bounds of one another); labels equal outside
the near-ties; (b) for all vertices the logits match the fp64 restatement within the bound and the labels match, near-ties at
most 2 %; (c) validate_scans_decoded's report equals get_seg_metrics on decode_scans' labels; (d) refine=10 equals refine_scans
afterwards; (e) a training-mode model, a bad val_whole and a first stage of another form raise; a VoteBatcher is decoded on its
`val` view; with the feature unused validate_scans' launches, batch()'s keys and the model's state are as before."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _scan_decode_ref as dref  # noqa: E402
import _seg_metrics_ref as sref  # noqa: E402
from _seg_metrics_ref import quiet  # noqa: E402
from test_scan_decode_gpu import _same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_cache = {}


# ---------------------------------------------------------------------------------------------------------------- model level
def _model_world():
    """The tiny eval model in WholePartSeg, the two scans as a set, one decode run with everything visible; made once."""
    if "world" not in _cache:
        from geot_amd.openpoints.dataset import DeviceScanSet, ValBatcher
        from geot_amd.openpoints.models.segmentation import WholePartSeg
        from geot_amd.validation import _decode_run
        scans = dref.tiny_scans()
        dset = DeviceScanSet([p for p, _ in scans], [l for _, l in scans], cls=[0, 1], device=DEV)
        seg = dref.tiny_model().to(DEV)
        model = WholePartSeg(segmentor_args=seg).eval()
        rng = np.random.default_rng(3)
        sel = np.stack([rng.choice(m, dref.N_SAMPLE, replace=False) for m in dref.SCAN_SIZES]).astype(np.int64)
        batcher = ValBatcher(dset, dref.N_SAMPLE)
        debug = []
        with torch.no_grad():
            preds, data = _decode_run(model, batcher, [0, 1], 17, None, 100, "test", debug=debug, sel=sel)      # three chunks
            f_l1, centres, _ = debug[0]["state"]
        torch.cuda.synchronize()
        n = lambda t: t.detach().cpu().numpy()
        rows = {k: np.concatenate([n(d[k]) for d in debug[1:]]) for k in ("q", "idx", "weight")}
        rows["logits"] = np.concatenate([n(d["logits"]).T for d in debug[1:]])             # (M0 + M1, C), slot after slot
        _cache["world"] = dict(dset=dset, seg=seg, model=model, sel=sel, batcher=batcher, data=data, scans=scans,
                               preds=[n(p).reshape(-1) for p in preds], forward=n(debug[0]["forward"]), rows=rows,
                               f_l1=n(f_l1), centres=n(centres), params=dref.stage_params(seg),
                               pos=n(data["pos"]), affine=[n(data[k]) for k in ("center", "scale", "view_center", "view_scale")])
    return _cache["world"]


def _restated(w, slot, q, idx, weight):
    return dref.last_stage(w["params"], w["f_l1"][slot], w["centres"][slot], slot, q, idx, weight)


def test_sampled_vertices_get_the_bits_of_pos_and_the_forward_logits():
    w = _model_world()
    starts = np.concatenate([[0], np.cumsum(dref.SCAN_SIZES)])
    excluded = total = 0
    for s in range(2):
        at = starts[s] + w["sel"][s]
        q = w["rows"]["q"][at]
        assert _same_bits(q, w["pos"][s])                                          # (a) q equals pos bit for bit
        d2, idx = dref.three_nn(q, w["centres"][s])
        assert np.array_equal(idx, w["rows"]["idx"][at]) and _same_bits(dref.fp_weights(d2), w["rows"]["weight"][at])
        want, bound = _restated(w, s, q, idx, dref.fp_weights(d2))
        fwd, dec = w["forward"][s].T, w["rows"]["logits"][at]
        e_f, e_d = np.abs(fwd - want) / bound, np.abs(dec - want) / bound
        print("slot %d sampled: forward error / bound %.3f, decoded %.3f, decoded - forward / summed bounds %.3f" %
              (s, e_f.max(), e_d.max(), (np.abs(dec - fwd) / (2 * bound)).max()))
        assert (e_f <= 1).all() and (e_d <= 1).all() and (np.abs(dec - fwd) <= 2 * bound).all()
        tie = dref.near_ties(want, bound)
        excluded, total = excluded + int(tie.sum()), total + len(tie)
        assert np.array_equal(w["preds"][s][w["sel"][s]][~tie], dref.argmax_rule(want)[~tie])
        assert np.array_equal(dref.argmax_rule(fwd)[~tie], dref.argmax_rule(want)[~tie])
    assert excluded / total <= dref.LABEL_CAP, (excluded, total)


def test_all_vertices_match_the_fp64_last_stage():
    w = _model_world()
    starts = np.concatenate([[0], np.cumsum(dref.SCAN_SIZES)])
    center, scale, vcenter, vscale = w["affine"]
    excluded = total = 0
    for s in range(2):
        rr = slice(starts[s], starts[s + 1])
        q = dref.query_positions(w["scans"][s][0], center[s], scale[s], vcenter[s], vscale[s])
        assert _same_bits(q, w["rows"]["q"][rr])
        d2, idx = dref.three_nn(q, w["centres"][s])
        weight = dref.fp_weights(d2)
        assert np.array_equal(idx, w["rows"]["idx"][rr]) and _same_bits(weight, w["rows"]["weight"][rr])
        want, bound = _restated(w, s, q, idx, weight)
        err = np.abs(w["rows"]["logits"][rr] - want) / bound
        print("slot %d all vertices: decoded error / bound %.3f (median bound %.2e)" % (s, err.max(), np.median(bound)))
        assert (err <= 1).all()
        tie = dref.near_ties(want, bound)
        excluded, total = excluded + int(tie.sum()), total + len(tie)
        assert np.array_equal(w["preds"][s][~tie], dref.argmax_rule(want)[~tie])
        assert np.array_equal(w["preds"][s], dref.argmax_rule(w["rows"]["logits"][rr]))   # the finish on the decoded logits
    print("near-ties left out: %d of %d" % (excluded, total))
    assert excluded / total <= dref.LABEL_CAP, (excluded, total)


def test_validators_agree_with_decode_scans_and_refine():
    from geot_amd.openpoints.dataset import ValBatcher
    from geot_amd.openpoints.dataset.sample_draw import DeviceDraws
    from geot_amd.validation import (SegMetrics, decode_scans, get_seg_metrics, refine_scans, seg_metrics_from_counts,
                                     validate_scans_decoded)
    w = _model_world()
    dset, model = w["dset"], w["model"]
    cfg = type("Cfg", (), {"num_classes": 17, "num_points": dref.N_SAMPLE, "epoch": 1, "epochs": 2})()
    fresh = lambda: ValBatcher(dset, dref.N_SAMPLE, draws=DeviceDraws(5))      # the same counter: the same batches
    preds = decode_scans(model, fresh(), [0, 1], chunk=100)
    labels = [torch.from_numpy(l).to(DEV) for _, l in w["scans"]]
    with quiet():
        got = validate_scans_decoded(model, fresh(), cfg, chunk=100)               # (c) the report of the same labels
        acc, miou, mdsc = get_seg_metrics(preds, labels, 17)
        rows = np.stack([dref.confusion_counts(p.cpu().numpy().reshape(-1), l, 17) for p, (_, l) in zip(preds, w["scans"])])
        want = seg_metrics_from_counts(rows, 17, [True, False])
    for g, key in zip(got, ("whole_macc", "whole_miou", "whole_mdsc")):
        assert np.asarray(g).dtype == np.asarray(want[key]).dtype and sref.same_value(g, want[key])
    assert all(sref.same_value(a, b) for a, b in zip(miou, want["miou_list"])) and all(sref.same_value(a, b) for a, b in zip(acc, want["acc_list"]))
    # a VoteBatcher is decoded on its `val` view (pos_search, whose affine batch(affine=True) hands out): the same samples, the
    # same view, the same labels, whatever the vote list does to pos
    from geot_amd.openpoints.dataset import VoteBatcher
    np.random.seed(2)
    torch.manual_seed(2)
    voted = decode_scans(model, VoteBatcher(dset, dref.N_SAMPLE, draws=DeviceDraws(5)), [0, 1], chunk=100)
    assert all(torch.equal(a, b) for a, b in zip(voted, preds))
    # (d) refine=10 is refine_scans applied afterwards
    refined = decode_scans(model, fresh(), [0, 1], refine=10, chunk=100)
    batch = fresh().batch([0, 1])
    after = refine_scans([p.clone() for p in preds], batch, 10, num_classes=17)
    assert all(torch.equal(a, b) for a, b in zip(refined, after))
    with quiet():
        got_r = validate_scans_decoded(model, fresh(), cfg, refine=10, chunk=100)
        m = SegMetrics(17, DEV)
        m.update(after, labels, [0, 1])
        want_r = m.read()
    assert all(sref.same_value(g, want_r[k]) for g, k in zip(got_r, ("whole_macc", "whole_miou", "whole_mdsc")))


def test_training_mode_and_bad_switches_raise():
    from geot_amd.fit import fit
    from geot_amd.openpoints.dataset import ValBatcher
    from geot_amd.validation import decode_scans
    w = _model_world()
    seg, model = w["seg"], w["model"]
    model.train()
    try:
        with pytest.raises(ValueError, match="eval mode"):
            decode_scans(model, ValBatcher(w["dset"], dref.N_SAMPLE), [0, 1])
        with pytest.raises(ValueError, match="eval mode"):
            seg.decode_front_params()
        with pytest.raises(ValueError, match="eval mode"):
            seg.decode_tail(torch.zeros(4, 128, device=DEV))
    finally:
        model.eval()
    with pytest.raises(ValueError, match="val_whole"):
        fit(None, None, {"val_whole": "direct", "epochs": 1})
    # a first stage that is not conv (no bias) -> BatchNorm -> ReLU
    first = list(seg.propogation_0.mlp.children())[0]
    bias = torch.nn.Parameter(torch.zeros(first.conv.out_channels, device=DEV))
    first.conv.bias = bias
    try:
        with pytest.raises(NotImplementedError, match="first stage"):
            seg._decode_first_stage()
        with pytest.raises(NotImplementedError, match="first stage"):
            decode_scans(model, ValBatcher(w["dset"], dref.N_SAMPLE), [0, 1])
        assert seg.decode_state is None and seg.keep_decode_state is False
    finally:
        first.conv.bias = None
    assert seg._decode_first_stage()[2] is True


def test_defaults_unchanged_when_the_feature_is_unused():
    """validate_scans' launches with the new calls unused: the same entry points, once per batch each, none of the new ones;
    batch()'s key set has no affine; the model keeps no decode state."""
    from geot_amd.ext import _common
    from geot_amd.openpoints.dataset import ValBatcher, VoteBatcher
    from geot_amd.validation import validate_scans
    w = _model_world()
    dset, model, seg = w["dset"], w["model"], w["seg"]
    cfg = type("Cfg", (), {"num_classes": 17, "num_points": dref.N_SAMPLE, "epoch": 1, "epochs": 2})()
    np.random.seed(4)
    with quiet():
        validate_scans(model, dset, cfg, batch_size=1)     # warm
    seen = []
    np.random.seed(4)
    _common.trace = lambda launch, name: (seen.append(name), launch())[1]
    try:
        with quiet():
            validate_scans(model, dset, cfg, batch_size=1)
    finally:
        _common.trace = None
    own = [s for s in seen if s in ("geot_cloud_sample_batch", "geot_fixmatch_views", "geot_view_program", "geot_scan_predict")]
    assert sorted(own) == sorted(["geot_cloud_sample_batch", "geot_fixmatch_views", "geot_scan_predict"] * 2), own
    assert own.count("geot_scan_predict") == 2 and not [s for s in seen if "decode" in s], seen
    assert seg.decode_state is None and seg.keep_decode_state is False
    np.random.seed(4)
    keys = set(ValBatcher(dset, dref.N_SAMPLE).batch([0, 1]))
    assert keys == {"pos", "x", "y", "cls", "center", "scale", "points", "labels", "scan_ids", "scans", "sizes", "mandible"}
    with_affine = ValBatcher(dset, dref.N_SAMPLE).batch([0, 1], affine=True)
    assert set(with_affine) == keys | {"view_center", "view_scale"}
    vote = VoteBatcher(dset, dref.N_SAMPLE, vote=[]).batch([0, 1], affine=True)
    assert set(vote) == keys | {"pos_search", "view_center", "view_scale"}
    assert tuple(with_affine["view_center"].shape) == (2, 3) and tuple(with_affine["view_scale"].shape) == (2,)
