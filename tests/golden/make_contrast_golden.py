"""Regenerate tests/golden/contrast_loss_ref.npz: the reference's ``nativeContrastLoss_t`` EXECUTED (build container only).

    python tests/golden/make_contrast_golden.py

As make_ntm_golden.py does it: the class definition is taken out of the reference's utils/cluster_contrastloss.py with
``ast``, compiled with the reference file as its filename and executed on the CPU with ``Tensor.cuda`` as the identity;
``torch.randperm`` is wrapped for the duration so that every permutation the class draws is recorded.  No reference source
text is written anywhere: the fixture holds the recorded permutations and results, the inputs are regenerated from the seed
(tests/_contrast_ref.py fixture_inputs / fixture_bank, which this script uses too).

Six consecutive calls on one object, B = 2, P = 96, D = 128, sample_nums = 16 (bank 64), th = 0.9 (:1390), the bank replaced
by the seeded one and the pointer started at 50 so that six calls reach both branches of _queue_operations.  Stored per
call i: perm_i (B, S) the first m entries of each cloud's permutation, perm_q_i (S), loss_i, grad_i (the feat_s gradient of
loss.backward()), bank_i and ptr_i after the call.  The class forces fp32 (.float() at :1224, :1259): these ARE fp32 results.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_ntm_golden as g  # noqa: E402
from _contrast_ref import FIXTURE, fixture_bank, fixture_inputs  # noqa: E402

SOURCE = "utils/cluster_contrastloss.py"


def main():
    assert os.path.isdir(g.REF), "run in the build container"
    f = FIXTURE
    b, s = f["B"], f["S"]
    ns = dict(torch=torch, nn=torch.nn, F=torch.nn.functional, np=np)
    g.ref_defs(SOURCE, ["nativeContrastLoss_t"], ns)
    drawn = []
    real = torch.randperm

    def recording(n, *a, **k):
        out = real(n, *a, **k)
        drawn.append(out.clone())
        return out

    out = {"bank0": fixture_bank()}
    seen_k, branches, any_short = set(), set(), False
    torch.manual_seed(f["seed"])
    with g.on_cpu(torch.float32):
        obj = ns["nativeContrastLoss_t"](sample_nums=s)
        obj.point_queue = torch.from_numpy(out["bank0"].copy())
        obj.point_queue_ptr = torch.full((1,), f["ptr0"], dtype=torch.long)
        torch.randperm = recording
        try:
            for call in range(len(f["K"])):
                feat_s, score, feat_t = (torch.from_numpy(a) for a in fixture_inputs(call))
                feat_s.requires_grad_(True)
                del drawn[:]
                before = int(obj.point_queue_ptr)
                loss = obj(feat_s, score, feat_t)[0]
                loss.backward()
                assert len(drawn) == b + 1 and [len(p) for p in drawn[:b]] == list(f["K"][call])
                perm = np.zeros((b, s), np.int64)
                total = 0
                for c in range(b):
                    m = min(len(drawn[c]), s)
                    perm[c, :m] = drawn[c][:m].numpy()
                    total += m
                    seen_k.add("<" if len(drawn[c]) < s else "=" if len(drawn[c]) == s else ">")
                assert len(drawn[b]) == total
                cnt = min(total, s)
                perm_q = np.zeros(s, np.int64)
                perm_q[:cnt] = drawn[b][:cnt].numpy()
                if before + cnt == 4 * s:
                    branches.add("exact")
                if before + cnt > 4 * s:
                    branches.add("past the end after cnt < S" if any_short else "past the end")
                any_short = cnt < s
                out.update({"perm_%d" % call: perm, "perm_q_%d" % call: perm_q, "loss_%d" % call: g.npf(loss),
                            "grad_%d" % call: g.npf(feat_s.grad), "bank_%d" % call: g.npf(obj.point_queue),
                            "ptr_%d" % call: np.int64(int(obj.point_queue_ptr))})
        finally:
            torch.randperm = real
    assert seen_k == {"<", "=", ">"}, seen_k
    assert branches == {"exact", "past the end after cnt < S"}, branches
    path = os.path.join(HERE, "contrast_loss_ref.npz")
    np.savez_compressed(path, meta=g.meta("inputs: tests/_contrast_ref.py fixture_inputs(call) / fixture_bank(), numpy "
                                          "default_rng((%d, call)); torch.manual_seed(%d) before the first call; pointer "
                                          "started at %d" % (f["seed"], f["seed"], f["ptr0"])), **out)
    print("%8.1f KB  %s" % (os.path.getsize(path) / 1024, os.path.basename(path)))
    assert os.path.getsize(path) <= 1 << 20


if __name__ == "__main__":
    main()
