"""Regenerate criteria_ref.npz: the four criteria train_one_epoch can be switched to, REFERENCE-EXECUTED (BUILD container
only: /root/reference does not exist on the GPU box).

    python tests/golden/make_criteria_golden.py

As make_ntm_golden.py does it: the class definitions of openpoints/loss/build.py are taken out of the reference file with
``ast``, compiled with that file as their filename and executed where they lie, on the CPU, once in fp32 and once with
torch's default dtype set to fp64; ``Tensor.cuda`` is the identity for the run (Poly1FocalLoss_U_T hard-codes ``.cuda()``,
build.py:658).  The fixture holds the small drawn inputs (labels, confidences, class weights), each loss and every input
gradient -- data only.  The two logits tensors are NOT stored: draw_inputs() rebuilds them from det_init.det_values, a
pure function of (name, index), on both sides.  N = 72 and one threshold, not more: twelve (B, C, N) gradients in fp32 and
fp64 are what the file is made of, and it has to stay smaller than val_batches_ref.npz.

    wce_bw2 / wce_bw3      Weight_CELoss            build.py:913-925   class_weights of 2 / 3 rows
    wceu_t095              Weight_CELoss_U          build.py:928-938   labels with one 255, confidence with one NaN
    pu_t095                Poly1FocalLoss_U         build.py:261-354   the same confidence
    put_t095               Poly1FocalLoss_U_T       build.py:564-688   gradients w.r.t. the logits AND pred_u_t

The conditions on the drawn inputs (check_inputs) are asserted here and again by tests/test_criteria_cpu.py, so that no
case can pass emptily.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from det_init import det_values  # noqa: E402

B, C, N = 2, 17, 72
THRESHOLDS = (("t095", 0.95),)
NAMES = ["Weight_CELoss", "Weight_CELoss_U", "Poly1FocalLoss_U", "Poly1FocalLoss_U_T"]


def draw_inputs():
    """The seeded inputs (a pure function of det_values: identical on every machine)."""
    logits = det_values("crit.logits", (B, C, N), 8.0)
    t = det_values("crit.t", (B, C, N), 8.0)                          # the second logits tensor of _U_T, both signs
    t = (np.sign(t) + (t == 0)) * np.clip(np.abs(t), 0.25, 4.0)       # |t| in [0.25, 4]: the reference divides by it
    labels = (det_values("crit.labels", (B, N), 1.0, 0.5) * C).astype(np.int64).clip(0, C - 1)
    labels[det_values("crit.bg", (B, N), 1.0, 0.5) < 0.15] = 0        # background: what Weight_CELoss_U drops by y == 0
    u, pick = det_values("crit.conf", (B, N), 1.0, 0.5), det_values("crit.mode", (B, N), 1.0, 0.5)
    conf = np.where(pick < 0.6, 0.96 + 0.04 * u, 0.3 + 0.6 * u).astype(np.float32)   # confident / not: a pseudo-label's
    conf_nan = conf.copy()
    labels_u = labels.copy()
    fg = np.argwhere((labels > 0) & (conf >= 0.95))
    (b0, n0), (b1, n1) = fg[3], fg[len(fg) // 2]
    conf_nan[b0, n0] = np.nan                                         # one NaN confidence on a foreground point
    labels_u[b1, n1] = 255                                            # one ignore label on a confident point
    cw2 = det_values("crit.cw2", (2, C), 0.1, 0.06)                   # tooth_dataset's class frequencies: small, positive
    cw3 = det_values("crit.cw3", (3, C), 0.1, 0.06)
    return dict(logits=logits, t=t.astype(np.float32), labels=labels, labels_u=labels_u, conf=conf, conf_nan=conf_nan,
                cw2=cw2, cw3=cw3)


def check_inputs(z, thresholds=tuple(v for _, v in THRESHOLDS)):
    """The conditions the issue sets on the inputs of the _U cases and of _U_T."""
    labels, labels_u, conf = z["labels"], z["labels_u"], z["conf_nan"]
    total = labels.size
    assert int((labels_u == 255).sum()) == 1 and int(np.isnan(conf).sum()) == 1
    assert not np.isnan(z["conf"]).any() and ((labels >= 0) & (labels < C)).all()
    with np.errstate(invalid="ignore"):
        for th in thresholds:
            confident = conf >= np.float32(th)
            kept = confident & (labels_u != 0) & (labels_u != 255)
            assert kept.sum() >= total / 4, ("kept", th, int(kept.sum()))
            assert (~confident).sum() >= total / 10, ("dropped by confidence", th)
            assert (confident & (labels_u == 0)).sum() >= total / 10, ("dropped by y == 0", th)
            assert (z["conf"] >= np.float32(th)).sum() >= total / 4           # _U_T's keep
    sel = np.take_along_axis(z["t"], labels[:, None, :], axis=1)[:, 0]
    assert (np.abs(sel) >= 0.25).all() and (np.abs(sel) <= 4.0).all() and (sel > 0).any() and (sel < 0).any()
    assert z["cw2"].shape == (2, C) and z["cw3"].shape == (3, C) and (z["cw2"] > 0).all() and (z["cw3"] > 0).all()


def main():
    from make_ntm_golden import DTYPES, LOSS, REF, base_namespace, meta, npf, on_cpu, ref_defs
    assert os.path.isdir(REF), "run in the build container"
    z = draw_inputs()
    check_inputs(z)
    ns = ref_defs(LOSS, NAMES, base_namespace())
    out = {k: v for k, v in z.items() if k not in ("logits", "t")}
    for dn, dt in DTYPES:
        with on_cpu(dt):
            def run(fn, *xs):
                """fn(*leaves) -> loss; -> the loss and the gradient of every leaf."""
                leaves = [torch.from_numpy(x).to(dt).requires_grad_(True) for x in xs]
                loss = fn(*leaves)
                loss.backward()
                return [npf(loss)] + [npf(x.grad) for x in leaves]
            lab, lab_u = torch.from_numpy(z["labels"]), torch.from_numpy(z["labels_u"])
            cf, cf_nan = torch.from_numpy(z["conf"]).to(dt), torch.from_numpy(z["conf_nan"]).to(dt)
            cases = {}
            for bw in (2, 3):
                cw = torch.from_numpy(z["cw%d" % bw]).to(dt)
                cases["wce_bw%d" % bw] = lambda cw=cw: run(lambda x: ns["Weight_CELoss"]()(x, lab, cw), z["logits"])
            cw2 = torch.from_numpy(z["cw2"]).to(dt)
            for tn, th in THRESHOLDS:
                # (Weight_CELoss_U writes 255 into the labels it is handed: a clone, as train.py:586 passes one)
                cases["wceu_" + tn] = lambda th=th: run(
                    lambda x: ns["Weight_CELoss_U"]()(x, lab_u.clone(), cw2, cf_nan.clone(), thresh=th), z["logits"])
                cases["pu_" + tn] = lambda th=th: run(
                    lambda x: ns["Poly1FocalLoss_U"]()(x, lab, cf_nan, thresh=th), z["logits"])
                cases["put_" + tn] = lambda th=th: run(
                    lambda x, t: ns["Poly1FocalLoss_U_T"]()(x, lab, cf, None, t, thresh=th), z["logits"], z["t"])
            for name, fn in cases.items():
                res = fn()
                out["%s_loss_%s" % (name, dn)] = res[0]
                out["%s_grad_%s" % (name, dn)] = res[1]
                if len(res) > 2:
                    out["%s_gradt_%s" % (name, dn)] = res[2]
                assert all(np.isfinite(r).all() for r in res), name
    path = os.path.join(HERE, "criteria_ref.npz")
    np.savez_compressed(path, meta=meta("B %d, C %d, N %d; thresholds %s; Tensor.cuda = identity" % (B, C, N, dict(THRESHOLDS))),
                        **out)
    print("%8.1f KB  %s" % (os.path.getsize(path) / 1024, os.path.basename(path)))


if __name__ == "__main__":
    main()
