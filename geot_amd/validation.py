"""The validation path of examples/segmentation/train.py:716-832.

``get_pred_whole`` (:781-800): per scan, de-normalise the N sampled points, take the 3 nearest sampled points of every
full-resolution vertex, inverse-distance interpolate the class probabilities and arg-max.  Same kernels as the training
path (three_nn / three_interpolate) at m ~ 1e5 unknown vertices; scans keep their own vertex counts, so the loop over
scans stays (each launch already fills the GPU).

``get_seg_metrics`` (:802-832), ``validate`` (:716-779) and ``SegMetrics``: the reference's per-scan accuracy, mIoU and
DSC and their jaw and whole means, from integer counts made on the device (csrc/seg_metrics.hip):

    metrics = SegMetrics(num_classes, device)
    for data in val_loader:                                  # collate_fn_val batches
        ...
        metrics.update_from_logits(logits, data["pos"], data["points"], data["center"], data["scale"], data["labels"], cls)
    out = metrics.read()                                     # one device-to-host copy: out["whole_miou"], out["miou_list"], ...
    metrics.reset()                                          # the next epoch

update_from_logits runs get_pred_whole's soft-max and three_nn, then interpolates, arg-maxes and counts in one launch per
batch: no (C, M) probabilities, no per-vertex prediction, no host synchronisation.  read() executes the reference's torch /
numpy statements on CPU int64 tensors built from the counts, so every value, NaN and dtype is the reference's.

With the test split resident on the device (openpoints.dataset.DeviceScanSet) no loader is needed either:

    out = validate_scans(model, scans, cfg)                  # validate()'s values from ValBatcher batches
    metrics.update_from_scans(logits, batch)                 # one geot_scan_predict call per batch, whatever its size
    preds = predict_scans(logits, batch)                     # get_pred_whole: the per-vertex labels of whole scans

geot_scan_predict (csrc/scan_predict.hip) reads the vertices and labels in place from the set, finds the three nearest
sampled points, interpolates, arg-maxes and counts / writes in one pass: no per-scan loop, no idx / dist2 in memory.

Test-time voting -- the config's `num_votes` and `datatransforms.vote`, which the reference carries and never uses: several
samples of the same scans, optionally under the vote transform list, the class probabilities of all passes interpolated onto
the whole scans and summed before the arg-max (geot_scan_vote: geot_scan_predict with a caller-owned accumulator):

    out = validate_scans_voted(model, scans, cfg)            # validate_scans with cfg.num_votes passes per batch
    preds = vote_scans(model, VoteBatcher(scans, n), idx, 10)    # the voted per-vertex labels of whole scans
    votes = ScanVotes(batch, num_classes); votes.add(logits, batch); ...; votes.add(logits, batch, last=True, want_pred=True)
    metrics.update_from_votes(votes, logits, batch)          # the last add(), counted into the epoch's rows

Covering passes -- every vertex predicted directly.  Independent samples cover a scan badly: at M = 100 000 vertices and
N = 16 000 samples a pass misses a vertex with probability 1 - N / M = 0.84, so after num_votes = 10 passes 0.84^10 = 17.5 % of
the vertices were never seen by the model, and every label is interpolated.  P = ceil(M / N) = 7 passes whose samples partition
the scan (geot_sample_draw_cover: consecutive windows of one permutation; ScanBatcher.cover) show it every vertex once, and
geot_scan_cover puts the model's probabilities on the very vertex a sample is -- no neighbour search, no interpolation:

    preds = cover_scans(model, ValBatcher(scans, n, draws=DeviceDraws(seed)), idx)           # P passes, each vertex its own value
    out = validate_scans_covered(model, scans, cfg, draws=DeviceDraws(seed))                 # validate()'s values from them
    cover = ScanCover(batch, num_classes); [cover.add(logits, batch, last=...) for batch in batcher.cover(idx)]

Refinement -- the config's `refine` and the reference's part_seg_refinement (train.py:57-73), which it defines and never
calls: the vertices of a class with fewer than n members in its scan, or of a class the jaw does not allow, take the majority
label of their n + 1 nearest vertices (geot_scan_refine, csrc/scan_refine.hip: six launches per batch, no synchronisation):

    preds = refine_scans(predict_scans(logits, batch), batch, n=10, parts=cls2parts)     # in place, the same views
    preds = predict_scans(logits, batch, refine=10)          # also vote_scans, validate_scans, validate_scans_voted
    pred = part_seg_refinement(pred, pos, cls, cls2parts, n=10)                         # the reference's dense (B, N) form

Decoding -- every vertex predicted directly from ONE forward pass.  Everything of PointTransformer_seg_T up to the features of
its 8192 centres depends on the sample alone; the last decoder stage (propogation_0, seg_head) is a pure function of a query's
position, and in eval mode nothing ties the query set to the sampled set.  geot_scan_decode_front (csrc/scan_decode.hip) takes
every vertex through the batch's two normalisations, finds its three nearest centres and writes the stage's first activations
point-major, chunk by chunk; the model's own code finishes the stage and the head, geot_scan_decode_finish takes the arg-max:

    preds = decode_scans(model, ValBatcher(scans, n), idx)                      # one batch(), one forward, then the chunks
    out = validate_scans_decoded(model, scans, cfg)                             # validate()'s values from them

These are the model's own decoder values at those positions; how decoded labels compare with interpolated or covered ones on
real scans has not been measured (there are no trained weights here).

Teeth3DS challenge scores -- TSA, TLA and TIR, what results on this dataset are published in (tooth_scores_from_moments has
the definitions).  Two of the three need geometry the confusion counts do not hold: geot_tooth_moments (csrc/tooth_scores.hip)
takes per scan and class the count, position sum and extent of the labelled and of the predicted vertices in one launch per
batch, integers only; every validator takes teeth= and sends each batch's final labels through it:

    teeth = ToothScores(num_classes, device)
    validate_scans(model, scans, cfg, teeth=teeth)           # also _voted, _covered, _decoded; the three-tuple as before
    out = teeth.read()                                       # one device-to-host copy: out["tsa"], out["tla"], out["tir"], out["score"]
    teeth.update(preds, batch)                               # any labels predict_scans / vote_scans / ... returned
    geo = tooth_instances(preds, batch, num_classes)         # per scan and class: predicted count, centroid, box (device tensors)

Connected teeth -- one FDI class in one jaw is one tooth, one connected patch of the surface, and nothing above enforces it:
every path labels each vertex on its own.  geot_scan_islands (csrc/scan_islands.hip: a lock-free union-find over a neighbour
table of the whole scan, six launches per batch, integers only) splits the labels into connected pieces and hands every stray
piece -- too small, of a class the jaw does not allow, or not the largest of its class -- to the label that surrounds it:

    preds = clean_scans(preds, batch, min_size=10, keep_largest=True, parts=cls2parts)   # in place, the same views
    comp = scan_components(preds, batch)                     # per vertex the first vertex of its piece
    preds = predict_scans(logits, batch, islands=True)       # also vote_scans, cover_scans, decode_scans, the validators, fit()
    result = teeth3ds_result(preds[0], comp[0], "lower")     # the challenge's labels (FDI) + instances, on the host

The table is each vertex's nearest vertices in space (scan_neighbours) or, for a set built with faces=, the scan mesh's own
one-ring (geot_mesh_neighbours, csrc/mesh_neighbours.hip: no search; two teeth in contact are not joined by it):

    table = mesh_neighbours(batch, k=16)                     # (sum M, 16) int32; clean_scans(..., mesh=True) builds it itself
    preds = predict_scans(logits, batch, islands={"mesh": True})
    scans.keep_tables()                                      # keep every scan's table of either kind on the set (off by default)

Look-ahead and replay -- validate_scans, validate_scans_voted and vote_scans with lookahead=G / graph=True (off by default):
up to G passes are drawn ahead (the same batch() calls in the same order), their coordinate-only work runs as one
prefetch_geometry over the concatenated positions beside the forward pass in flight (pass_schedule, _passes), and with graph
that call and the forward pass replay from hipGraphs (graph_eval.GraphedForward).  Same values, bit for bit:

    out = validate_scans_voted(model, scans, cfg, graph=True, lookahead=True)    # one FPS launch per group of num_votes passes
"""
import logging

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib, graph_eval, streams
from .ext._common import call, knn_workspace, need, ptr
from .openpoints.dataset.scan_set import _to_device
from .pointnet2 import pointnet2_utils as pt_utils

MAX_VERTICES = (1 << 31) - 1        # per scan (include/geot_hip.h geot_seg_confusion)
# geot_scan_predict's work table.  A wave is serial over its vertices, so the table decides how many waves a launch has: an
# MI355X holds 256 CUs x 4 SIMDs x 8 waves = 8192 waves of this kernel (occupancy 8), and knn_grid_kernel, which the search
# comes from, gives every query a wave of its own.  4096 workgroups of 4 waves are two rounds of the full device; below
# ~2.6e5 vertices the floor of 64 vertices per workgroup (16 per wave) applies instead, which at B = 2, M ~1e5 gives ~3100
# workgroups = ~12 400 waves.  Against that stands the per-workgroup cost (clearing and flushing 4 x (C (C + 1) + 1) LDS
# counters, one grid header).  Measured at B = 2, M ~1e5, N = 16 000 (profiles/validation_resident.txt, device time of one
# update): 64 vertices per workgroup 0.355 ms, 32: 0.338, 16: 0.358, 128: 0.383, 256: 0.474; 2048 / 1024 / 512 groups with the
# floor of 64: 0.364 / 0.389 / 0.531.  One run at one size: the constants stay at the values the tests and the recorded
# verdict were run with; 32 per workgroup is the candidate.
SCAN_GROUPS = 4096
SCAN_CHUNK_MIN = 64
SCAN_MAX_SLOTS = 65535              # batch slots per call (include/geot_hip.h geot_scan_predict)
REFINE_MAX_N = 63                   # include/geot_hip.h geot_scan_refine: n + 1 neighbours in one wave's list


def _need_classes(num_classes, what):
    c = int(num_classes)
    need(1 <= c <= _lib.NTM_MAX_C, "%s: 1..%d classes (include/geot_hip.h GEOT_NTM_MAX_C), got %d" % (what, _lib.NTM_MAX_C, c))
    return c


def _refine_n(n, what, keyword=True):
    """Refine's n: an int, no bool, in 1 .. REFINE_MAX_N.  keyword: the `refine` keyword of predict_scans, vote_scans and the
    validators, which is also 0 / False / None -> 0 (off) or True -> 10 (the reference's default n)."""
    if keyword and (n is None or isinstance(n, bool)):
        return 10 if n else 0
    need(isinstance(n, (int, np.integer)) and not isinstance(n, bool) and (0 if keyword else 1) <= int(n) <= REFINE_MAX_N,
         "%s: %s must be an int in 1..%d%s, got %r" % (what, "refine" if keyword else "n", REFINE_MAX_N, " (0: off)" if keyword else "", n))
    return int(n)


def _three_nn_inputs(points, points_whole, center, scale, index, dev):
    """get_pred_whole's statements for scan `index` up to its three_nn call -> (unknown (1, M, 3), known (1, N, 3)), fp32."""
    point = points[index].unsqueeze(0).contiguous()
    s = torch.as_tensor(scale[index]).to(dev).unsqueeze(0).contiguous()
    c = torch.as_tensor(center[index]).to(dev).unsqueeze(0).contiguous()
    point_whole = torch.as_tensor(points_whole[index]).to(dev).unsqueeze(0).contiguous()
    point = (point * s + c).contiguous()
    return point_whole.float().contiguous(), point.float().contiguous()


@torch.no_grad()
def get_pred_whole(logits, points, points_whole, center, scale):
    """logits (B,C,N); points (B,N,3) normalised; points_whole: list of (M_i,3); center/scale: per-scan
    tensors broadcastable to (1,N,3) -> list of (1, M_i) int64 predicted labels."""
    logits = F.softmax(logits, dim=1)
    dev = logits.device
    preds_whole = []
    for index in range(logits.shape[0]):
        logit = logits[index].unsqueeze(0).contiguous()
        dist, idx = pt_utils.three_nn(*_three_nn_inputs(points, points_whole, center, scale, index, dev))
        dist_recip = 1.0 / (dist + 1e-8)
        weight = dist_recip / torch.sum(dist_recip, dim=2, keepdim=True)
        logit_whole = pt_utils.three_interpolate(logit, idx, weight)
        preds_whole.append(logit_whole.argmax(dim=1))
    return preds_whole


def seg_metrics_from_counts(counts, num_classes, mandible):
    """read()'s host half (no device needed): counts (S, C (C + 1) + 1) int64 laid out as geot_seg_confusion writes them,
    mandible (S,) the jaw of every scan (validate's `cls[ii] == 0`) -> the dict SegMetrics.read() returns.  The reference's
    statements run on CPU int64 tensors made from the counts: get_seg_metrics (train.py:811-830) per scan, validate's
    aggregation (:747-763).  A label outside [0, C) raises: the reference's result would depend on how many distinct
    such values there were, which the counts do not keep."""
    c = int(num_classes)
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, c * (c + 1) + 1)
    need(len(mandible) == counts.shape[0], "SegMetrics: %d jaw flags for %d scans" % (len(mandible), counts.shape[0]))
    bad = int(counts[:, -1].sum())
    if bad:
        raise RuntimeError("SegMetrics: %d labels outside [0, %d) this epoch" % (bad, c))
    acc_list, miou_list, mdsc_list = [], [], []
    for row in counts:
        conf = row[:-1].reshape(c, c + 1)           # (label, prediction); column c = prediction outside [0, C)
        n_label, n_pred, hit = conf.sum(1), conf[:, :c].sum(0), np.diagonal(conf)
        iou, dsc = [], []
        for jcls in range(1, c):                    # torch.unique(label) in ascending order, class 0 skipped
            if n_label[jcls] == 0:
                continue
            jcls_and = torch.tensor(int(hit[jcls]))
            jcls_or = torch.tensor(int(n_pred[jcls] + n_label[jcls] - hit[jcls]))
            iou.append((jcls_and / jcls_or).float())
            dsc.append((2 * iou[-1] / (1 + iou[-1])))
        acc = torch.tensor(int(hit.sum())) / int(n_label.sum())
        acc_list.append(acc)
        miou_list.append(np.array(iou).mean())
        mdsc_list.append(np.array(dsc).mean())
    out = dict(acc_list=acc_list, miou_list=miou_list, mdsc_list=mdsc_list, scans=len(acc_list), labels_out_of_range=bad)
    jaws = {}
    for jaw, lower in (("mandible", True), ("maxillary", False)):
        sel = [i for i, m in enumerate(mandible) if bool(m) == lower]
        jaws[jaw] = {k: [lst[i] for i in sel] for k, lst in (("acc", acc_list), ("miou", miou_list), ("dsc", mdsc_list))}
        out[jaw + "_macc"] = np.array(jaws[jaw]["acc"]).mean()
        out[jaw + "_miou"] = np.array(jaws[jaw]["miou"]).mean()
        out[jaw + "_mdsc"] = np.array(jaws[jaw]["dsc"]).mean()
    lo, up = jaws["mandible"], jaws["maxillary"]
    for key, name in (("acc", "whole_macc"), ("miou", "whole_miou"), ("dsc", "whole_mdsc")):
        out[name] = (np.array(lo[key]).sum() + np.array(up[key]).sum()) / (len(lo[key]) + len(up[key]))
    return out


def scan_work_table(sizes, groups=SCAN_GROUPS, min_chunk=SCAN_CHUNK_MIN):
    """geot_scan_predict's work table for batch slots of `sizes` vertices -> (G, 4) int32 host array of (slot, first vertex,
    vertex count, 0): every scan cut into chunks of one common length -- a multiple of 4 (one quarter per wave), at least
    min_chunk, about sum(sizes) / groups -- so that ragged scans share the device evenly; the last chunk of a scan is the
    remainder.  Every vertex of every slot lies in exactly one entry.  G <= groups + len(sizes)."""
    sizes = [int(m) for m in sizes]
    need(all(1 <= m <= MAX_VERTICES for m in sizes), "scan_work_table: 1 .. %d vertices per scan" % MAX_VERTICES)
    need(int(groups) >= 1 and int(min_chunk) >= 1, "scan_work_table: groups >= 1 and min_chunk >= 1")
    total = sum(sizes)
    chunk = max(int(min_chunk), -(-total // int(groups)))
    chunk = min(-(-chunk // 4) * 4, MAX_VERTICES)
    rows = []
    for slot, m in enumerate(sizes):
        first = np.arange(0, m, chunk, dtype=np.int64)
        part = np.zeros((first.size, 4), dtype=np.int64)
        part[:, 0], part[:, 1], part[:, 2] = slot, first, np.minimum(chunk, m - first)
        rows.append(part)
    table = np.concatenate(rows) if rows else np.zeros((0, 4), dtype=np.int64)
    return np.ascontiguousarray(table.astype(np.int32))


def _scan_inputs(logits, batch, num_classes, what, pos_key="pos"):
    """The checks of one whole-scan call on a ValBatcher batch, then get_pred_whole's soft-max and de-normalisation as batched
    torch statements (the same fp32 multiply and add per element as its per-scan `point * s + c`)
    -> (b, n, scan_ids, prob (B, C, N), known (B, N, 3))."""
    need(isinstance(batch, dict) and all(k in batch for k in (pos_key, "center", "scale", "scan_ids", "scans", "sizes")),
         "%s: batch must come from ValBatcher.batch (%s, center, scale, scan_ids, scans, sizes)" % (what, pos_key))
    scans, sizes = batch["scans"], [int(m) for m in batch["sizes"]]
    dev = scans.device
    c = int(num_classes)
    need(torch.is_tensor(logits), "%s: logits must be a torch.Tensor" % what)
    need(logits.is_cuda, "%s: CPU not supported (logits must live on the GPU)" % what)
    need(logits.dim() == 3 and logits.shape[1] == c and logits.dtype == torch.float32, "%s: fp32 logits (B, %d, N)" % (what, c))
    need(logits.device == dev, "%s: logits on %s, the scans on %s" % (what, logits.device, dev))
    b, _, n = logits.shape
    need(b == len(sizes) and 1 <= b <= SCAN_MAX_SLOTS, "%s: %d logits rows for a batch of %d scans (1 .. %d)" %
         (what, b, len(sizes), SCAN_MAX_SLOTS))
    need(all(torch.is_tensor(batch[k]) for k in (pos_key, "center", "scale", "scan_ids")), "%s: batch %s, center, scale and scan_ids "
         "must be tensors" % (what, pos_key))
    need(n >= 1 and tuple(batch[pos_key].shape) == (b, n, 3), "%s: logits (B, C, N) and batch %s (B, N, 3) must agree, N >= 1" %
         (what, pos_key))
    need(tuple(batch["center"].shape) == (b, 3) and tuple(batch["scale"].shape) == (b,) and tuple(batch["scan_ids"].shape) == (b,),
         "%s: batch center (B, 3), scale (B,), scan_ids (B,)" % what)
    for key, dt in ((pos_key, torch.float32), ("center", torch.float32), ("scale", torch.float32), ("scan_ids", torch.int64)):
        need(torch.is_tensor(batch[key]) and batch[key].device == dev and batch[key].dtype == dt,
             "%s: batch %s must be a %s tensor on %s" % (what, key, dt, dev))
    scan_ids = batch["scan_ids"].contiguous()
    prob = F.softmax(logits, dim=1).contiguous()
    known = (batch[pos_key] * batch["scale"].view(b, 1, 1) + batch["center"].view(b, 1, 3)).contiguous()
    return b, n, scan_ids, prob, known


def _out_offsets(sizes, dev):
    """Where every slot's vertices start in a per-vertex output laid out slot after slot: (b,) int64 on the device."""
    ends = np.cumsum(sizes, dtype=np.int64)
    return _to_device(np.concatenate([[0], ends[:-1]]).astype(np.int64), dev)


def _scan_launch(logits, batch, num_classes, what, counts=None, want_pred=False, votes=None, mode=0):
    """One geot_scan_predict call for a ValBatcher batch -- for a ScanVotes, one geot_scan_vote call on its accumulator, work
    table and out_offsets, searching batch["pos_search"] when the batch has one: _scan_inputs, the workspace, the kernel
    -> the per-vertex labels as a list of (1, M_i) int64 views of one buffer, or None without want_pred."""
    pos_key = "pos_search" if votes is not None and isinstance(batch, dict) and "pos_search" in batch else "pos"
    b, n, scan_ids, prob, known = _scan_inputs(logits, batch, num_classes, what, pos_key)
    scans, sizes = batch["scans"], [int(m) for m in batch["sizes"]]
    dev = scans.device
    if votes is not None:
        need(scans is votes.scans and sizes == votes.sizes, "%s: every vote's batch holds the same scans in the same slots" % what)
        work, out_offs = votes.work, votes.out_offsets
    else:                               # the un-voted call builds its tables per call, out_offsets only for the labels
        work = _to_device(scan_work_table(sizes), dev)
        out_offs = _out_offsets(sizes, dev) if want_pred else None
    pred = torch.empty(sum(sizes), dtype=torch.int64, device=dev) if want_pred else None
    nbytes = int(_lib.load().geot_scan_predict_ws_bytes(b, n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    entry, acc = ("geot_scan_predict", ()) if votes is None else ("geot_scan_vote", (ptr(votes.acc), mode))
    call(entry, dev, b, int(num_classes), n, len(scans), int(scans.points.shape[0]), ptr(scans.points), ptr(scans.labels),
         ptr(scans.offsets), ptr(scan_ids), ptr(known), ptr(prob), int(work.shape[0]), ptr(work), ptr(out_offs), *acc,
         ptr(pred), ptr(counts), ptr(ws), nbytes)
    return [p.view(1, -1) for p in torch.split(pred, sizes)] if want_pred else None


@torch.no_grad()
def predict_scans(logits, batch, refine=0, parts=None, islands=None):
    """The per-vertex labels of the batch's whole scans: list of (1, M_i) int64 tensors (views of one buffer), equal to
    get_pred_whole(logits, batch["pos"], batch["points"], batch["center"], batch["scale"]).  logits (B, C, N) fp32 on the
    scans' device, batch from ValBatcher.batch.  One geot_scan_predict call, no host synchronisation.  refine (0: off, True:
    n = 10, an int: n) and parts: the labels then go through refine_scans.  islands (None / False: off, True: clean_scans'
    defaults, a dict: its keyword arguments; anything else is a ValueError before any device call): the labels then, after
    refine, go through clean_scans."""
    n_refine = _refine_n(refine, "predict_scans")
    islands = _islands_kw(islands, "predict_scans")
    if isinstance(batch, dict):
        _need_mesh(islands, batch.get("scans"), "predict_scans")
    need(torch.is_tensor(logits) and logits.dim() == 3, "predict_scans: logits must be a (B, C, N) tensor")
    preds = _scan_launch(logits, batch, logits.shape[1], "predict_scans", want_pred=True)
    return _finish_labels(preds, batch, n_refine, parts, islands, logits.shape[1])


def _allowed_masks(parts, jaws, c, what):
    """parts (the reference's cls2parts: per jaw class the allowed labels) and the slots' jaw classes -> one bit mask per slot."""
    masks = []
    for row in parts:
        labels = [int(l) for l in row]
        need(all(0 <= l < c for l in labels), "%s: parts must hold labels in [0, %d)" % (what, c))
        masks.append(sum(1 << l for l in set(labels)))
    need(all(0 <= j < len(masks) for j in jaws), "%s: parts has %d rows, the jaw classes are %s" % (what, len(masks), sorted(set(jaws))))
    return np.array([masks[j] for j in jaws], dtype=np.uint32)


def _scan_refine(pred, n, c, points, offsets, scan_ids, n_scans, out_offs, allowed, b, want_stats):
    """One geot_scan_refine call on the flat int64 label buffer `pred`; allowed: _allowed_masks' host array, or None."""
    dev = pred.device
    allowed = _to_device(allowed.view(np.int32), dev) if allowed is not None else None
    nbytes = int(_lib.load().geot_scan_refine_ws_bytes(b, int(pred.numel()), n))
    need(nbytes >= 0, "geot_scan_refine: no workspace for b = %d, n = %d, %d labels" % (b, n, pred.numel()))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stats = torch.empty((b, 4), dtype=torch.int32, device=dev) if want_stats else None
    call("geot_scan_refine", dev, b, c, n, n_scans, int(points.shape[0]), ptr(points), ptr(offsets), ptr(scan_ids), ptr(out_offs),
         ptr(allowed), ptr(pred), ptr(stats), ptr(ws), nbytes)
    return stats


def _flat_labels(preds, sizes, dev):
    """Per-scan int64 label tensors as one flat buffer, slot after slot -> (flat, views): the very memory when they are
    contiguous views of one buffer in that order (what predict_scans and its kin return; views = True), a concatenated copy
    otherwise."""
    at, views = preds[0].storage_offset(), True
    for p, m in zip(preds, sizes):
        views = (views and p.is_contiguous() and p.untyped_storage().data_ptr() == preds[0].untyped_storage().data_ptr()
                 and p.storage_offset() == at)
        at += m
    if views:
        return torch.empty(0, dtype=torch.int64, device=dev).set_(preds[0].untyped_storage(), preds[0].storage_offset(), (sum(sizes),), (1,)), True
    return torch.cat([p.reshape(-1) for p in preds]), False


@torch.no_grad()
def refine_scans(preds, batch, n=10, parts=None, stats=False, num_classes=None):
    """part_seg_refinement (train.py:57-73) on whole scans: preds as predict_scans / vote_scans return them -- per scan of the
    batch a (1, M_i) int64 tensor -- refined IN PLACE when they are views of one buffer, slot after slot (a list that is not is
    concatenated and split again); returns the list, with stats=True (list, (B, 4) int32 device tensor of steps, queries,
    changed vertices, labels outside [0, C) per scan).  Per scan: a class with fewer than n vertices, or one that parts does
    not allow for the scan's jaw, hands its vertices to the majority label of their n + 1 nearest vertices (the class itself
    excluded, the lowest label among equals); classes in the order of their first vertex, every class's queries taken from the
    labels as they came in.  parts: None (every class allowed) or, per jaw class (0 mandible, 1 maxillary, from
    batch["mandible"]), the allowed labels -- the reference's cls2parts.  num_classes: default parts[-1][-1] + 1 as in the
    reference, 32 without parts.  One geot_scan_refine call, no host synchronisation."""
    n = _refine_n(n, "refine_scans", keyword=False)
    need(isinstance(batch, dict) and all(k in batch for k in ("scan_ids", "scans", "sizes")),
         "refine_scans: batch must come from ValBatcher.batch (scan_ids, scans, sizes)")
    scans, sizes = batch["scans"], [int(m) for m in batch["sizes"]]
    b = len(sizes)
    need(isinstance(preds, (list, tuple)) and len(preds) == b and 1 <= b <= SCAN_MAX_SLOTS,
         "refine_scans: one prediction tensor per scan of the batch (1 .. %d)" % SCAN_MAX_SLOTS)
    for p, m in zip(preds, sizes):
        need(torch.is_tensor(p) and p.dtype == torch.int64, "refine_scans: the predictions must be int64 tensors")
        need(p.numel() == m, "refine_scans: %d predictions for a scan of %d vertices" % (p.numel(), m))
        need(m >= n + 1, "refine_scans: a scan of %d vertices has no %d nearest vertices (n + 1)" % (m, n + 1))
    if num_classes is None:
        num_classes = 32 if parts is None else int(parts[-1][-1]) + 1
    c = _need_classes(num_classes, "refine_scans")
    allowed = None
    if parts is not None:
        need("mandible" in batch and len(batch["mandible"]) == b, "refine_scans: parts needs the batch's jaw flags (mandible)")
        allowed = _allowed_masks(parts, [0 if m else 1 for m in batch["mandible"]], c, "refine_scans")
    dev = scans.device
    need(all(p.is_cuda and p.device == dev for p in preds), "refine_scans: CPU not supported (the predictions must live on %s, "
         "with the scans)" % dev)
    need(torch.is_tensor(batch["scan_ids"]) and batch["scan_ids"].device == dev and batch["scan_ids"].dtype == torch.int64 and
         tuple(batch["scan_ids"].shape) == (b,), "refine_scans: batch scan_ids must be (B,) int64 on %s" % dev)
    flat, views = _flat_labels(preds, sizes, dev)
    out = list(preds) if views else [f.view(p.shape) for f, p in zip(torch.split(flat, sizes), preds)]
    st = _scan_refine(flat, n, c, scans.points, scans.offsets, batch["scan_ids"].contiguous(), len(scans), _out_offsets(sizes, dev),
                      allowed, b, stats)
    return (out, st) if stats else out


@torch.no_grad()
def part_seg_refinement(pred, pos, cls, cls2parts, n=10):
    """train.py:57-73 with the reference's signature: pred (B, N) int64 and pos (B, N, 3) fp32 on the GPU, cls the B shape
    classes (rows of cls2parts), cls2parts per shape class the allowed labels; the class count is cls2parts[-1][-1] + 1.
    pred is refined in place and returned.  The reference's rule for the CUDA tensors it is written for: the labels are
    snapshotted before anything changes.  The same geot_scan_refine call as refine_scans, every row a scan of N vertices."""
    n = _refine_n(n, "part_seg_refinement", keyword=False)
    need(torch.is_tensor(pred) and torch.is_tensor(pos), "part_seg_refinement: pred and pos must be tensors")
    need(pred.dtype == torch.int64 and pred.dim() == 2, "part_seg_refinement: pred must be (B, N) int64")
    bsz, npts = pred.shape
    need(pos.dtype == torch.float32 and tuple(pos.shape) == (bsz, npts, 3), "part_seg_refinement: pos must be (B, N, 3) fp32")
    need(npts >= n + 1, "part_seg_refinement: %d points have no %d nearest points (n + 1)" % (npts, n + 1))
    need(1 <= bsz <= SCAN_MAX_SLOTS, "part_seg_refinement: 1 .. %d shapes" % SCAN_MAX_SLOTS)
    c = _need_classes(int(cls2parts[-1][-1]) + 1, "part_seg_refinement")
    jaws = [int(j) for j in (cls.detach().cpu().reshape(-1).tolist() if torch.is_tensor(cls) else np.asarray(cls).reshape(-1))]
    need(len(jaws) == bsz, "part_seg_refinement: %d shape classes for %d shapes" % (len(jaws), bsz))
    allowed = _allowed_masks(cls2parts, jaws, c, "part_seg_refinement")
    need(pred.is_cuda and pos.is_cuda and pred.device == pos.device, "part_seg_refinement: CPU not supported (pred and pos must "
         "live on one GPU)")
    need(pred.is_contiguous(), "part_seg_refinement: pred must be contiguous (it is refined in place)")
    dev = pred.device
    offsets = _to_device(np.arange(bsz + 1, dtype=np.int64) * npts, dev)
    ids = _to_device(np.arange(bsz, dtype=np.int64), dev)
    _scan_refine(pred.view(-1), n, c, pos.contiguous().view(-1, 3), offsets, ids, bsz, offsets[:bsz], allowed, bsz, False)
    return pred


# ---- connected pieces of whole-scan labels, stray islands relabelled (csrc/scan_islands.hip) ----------------------------------------
ISLANDS_MAX_K = 32                  # include/geot_hip.h geot_scan_islands: entries per row of the neighbour table
MESH_K = 16                         # mesh_neighbours' default width, and what mesh=True means
_CLEAN_KEYS = ("min_size", "keep_largest", "parts", "nbr", "k", "num_classes", "mesh")


def _mesh_width(mesh, what, error=RuntimeError):
    """The `mesh` keyword of clean_scans and scan_components -> None (None or False: the kNN table) or the width of the mesh
    table (True: MESH_K; an int in 1..32: that)."""
    if mesh is None or mesh is False:
        return None
    if mesh is True:
        return MESH_K
    if not isinstance(mesh, (int, np.integer)) or not 1 <= int(mesh) <= ISLANDS_MAX_K:
        raise error("%s: mesh must be None, a bool or an int in 1..%d (the width of the one-ring table), got %r" % (what, ISLANDS_MAX_K, mesh))
    return int(mesh)


def _clean_args(min_size, keep_largest, k, what, error=RuntimeError):
    """clean_scans' host-only arguments -> (min_size, keep: True or a sorted tuple of classes, k)."""
    def refuse(msg):
        raise error("%s: %s" % (what, msg))
    if isinstance(min_size, bool) or not isinstance(min_size, (int, np.integer)) or int(min_size) < 0:
        refuse("min_size must be an int >= 0, got %r" % (min_size,))
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= ISLANDS_MAX_K - 1:
        refuse("k must be an int in 1..%d (the table holds k + 1 entries per vertex), got %r" % (ISLANDS_MAX_K - 1, k))
    if isinstance(keep_largest, bool):
        keep = keep_largest
    else:
        try:
            keep = tuple(sorted(set(keep_largest)))
        except TypeError:
            refuse("keep_largest must be a bool or an iterable of classes, got %r" % (keep_largest,))
        if not all(isinstance(i, (int, np.integer)) and not isinstance(i, bool) and 0 <= int(i) < _lib.NTM_MAX_C for i in keep):
            refuse("keep_largest must name classes in [0, %d), got %r" % (_lib.NTM_MAX_C, keep_largest))
        keep = tuple(int(i) for i in keep)
    return int(min_size), keep, int(k)


def _islands_kw(islands, what):
    """The `islands` keyword of predict_scans, vote_scans, cover_scans, decode_scans, the validators and fit(), checked before
    any device call -> None (off: None or False) or the keyword arguments of clean_scans (True: {}, the defaults; a dict: its
    items).  Anything else, an unknown key or a value clean_scans would refuse on the host: ValueError."""
    if islands is None or islands is False:
        return None
    if islands is True:
        return {}
    if not isinstance(islands, dict):
        raise ValueError("%s: islands must be None, a bool or a dict of clean_scans' keyword arguments, got %r" % (what, islands))
    unknown = sorted(str(key) for key in islands if key not in _CLEAN_KEYS)
    if unknown:
        raise ValueError("%s: islands has no keyword %s (clean_scans takes %s)" % (what, ", ".join(unknown), ", ".join(_CLEAN_KEYS)))
    _clean_args(islands.get("min_size", 10), islands.get("keep_largest", True), islands.get("k", 8), what + ": islands", ValueError)
    if _mesh_width(islands.get("mesh"), what + ": islands", ValueError) is not None and islands.get("nbr") is not None:
        raise ValueError("%s: islands gives both mesh and nbr (one table or the other)" % what)
    return dict(islands)


def _need_mesh(islands, scans, what):
    """islands={"mesh": ...} on a set without faces: ValueError before the first forward pass (scans: the set, or a batcher)."""
    if islands is not None and _mesh_width(islands.get("mesh"), what, ValueError) is not None:
        if getattr(getattr(scans, "scans", scans), "faces", None) is None:
            raise ValueError("%s: islands asks for the mesh table (mesh=%r) and the scan set holds no faces -- build it with "
                             "DeviceScanSet(..., faces=)" % (what, islands["mesh"]))


def _islands_batch(preds, batch, what):
    """The checks clean_scans, scan_components and scan_neighbours share with refine_scans -> (scans, sizes, b, dev)."""
    need(isinstance(batch, dict) and all(key in batch for key in ("scan_ids", "scans", "sizes")),
         "%s: batch must come from ValBatcher.batch (scan_ids, scans, sizes)" % what)
    scans, sizes = batch["scans"], [int(m) for m in batch["sizes"]]
    b = len(sizes)
    need(1 <= b <= SCAN_MAX_SLOTS, "%s: 1 .. %d scans per batch" % (what, SCAN_MAX_SLOTS))
    if preds is not None:
        need(isinstance(preds, (list, tuple)) and len(preds) == b, "%s: one prediction tensor per scan of the batch" % what)
        for p, m in zip(preds, sizes):
            need(torch.is_tensor(p) and p.dtype == torch.int64, "%s: the predictions must be int64 tensors" % what)
            need(p.numel() == m, "%s: %d predictions for a scan of %d vertices" % (what, p.numel(), m))
    dev = scans.device
    if preds is not None:
        need(all(p.is_cuda and p.device == dev for p in preds), "%s: CPU not supported (the predictions must live on %s, with "
             "the scans)" % (what, dev))
    need(torch.is_tensor(batch["scan_ids"]) and batch["scan_ids"].device == dev and batch["scan_ids"].dtype == torch.int64 and
         tuple(batch["scan_ids"].shape) == (b,), "%s: batch scan_ids must be (B,) int64 on %s" % (what, dev))
    return scans, sizes, b, dev


def _scan_rows(batch, sizes, dev):
    """Per slot the (M_s, 3) fp32 vertices of its scan: the batcher's zero-copy views when the batch carries them (read in
    place), else gathered from the set on the device by the slots' scan ids.  No synchronisation either way."""
    scans = batch["scans"]
    views = batch.get("points")
    if (isinstance(views, (list, tuple)) and len(views) == len(sizes) and
            all(torch.is_tensor(p) and p.device == dev and p.dtype == torch.float32 and tuple(p.shape) == (m, 3) and p.is_contiguous()
                for p, m in zip(views, sizes))):
        return list(views)
    b, total = len(sizes), sum(sizes)
    slot = torch.repeat_interleave(torch.arange(b, device=dev), _to_device(np.asarray(sizes, dtype=np.int64), dev), output_size=total)
    first = scans.offsets[batch["scan_ids"]] - _out_offsets(sizes, dev)
    return list(torch.split(scans.points[first[slot] + torch.arange(total, device=dev)], sizes))


@torch.no_grad()
def scan_neighbours(batch, k=8):
    """The neighbour table of the batch's whole scans: (sum M, k + 1) int32 on the device, slot after slot -- per vertex its
    k + 1 nearest vertices of the same scan as indices local to the scan, itself included, in geot_knn_sorted's (d2, index)
    order.  One geot_knn_sorted_ws call per slot (b = 1, nq = nr = M_s; the grid search at whole-scan sizes) on the scan's rows
    of scans.points, read in place from the batcher's views; the sizes are the host's.  A scan of fewer than k + 1 vertices is
    refused, so the table never holds the search's filler.  By default nothing is cached and a scan met again is searched
    again; after scans.keep_tables() every scan's table is kept on the set, only the missing ones are searched and the batch's
    table is assembled from the kept ones (DeviceScanSet.keep_tables: the same bits, 4 (k + 1) M_i bytes per scan)."""
    scans, sizes, b, dev = _islands_batch(None, batch, "scan_neighbours")
    _, _, k = _clean_args(0, False, k, "scan_neighbours")
    for m in sizes:
        if m < k + 1:
            raise ValueError("scan_neighbours: a scan of %d vertices has no %d nearest vertices (k + 1)" % (m, k + 1))
    need(scans.points.is_cuda, "scan_neighbours: CPU not supported (the scans must live on the GPU)")
    return _kept_or_built(batch, sizes, dev, "knn", k + 1, lambda part, part_sizes: (_knn_tables(part, part_sizes, dev, k), None))[0]


def _knn_tables(batch, sizes, dev, k):
    """scan_neighbours' searches: one geot_knn_sorted_ws call per slot."""
    rows = _scan_rows(batch, sizes, dev)
    nbr = torch.empty((sum(sizes), k + 1), dtype=torch.int32, device=dev)
    dist2 = torch.empty((max(sizes), k + 1), dtype=torch.float32, device=dev)       # the search writes it; nobody reads it
    at = 0
    for p, m in zip(rows, sizes):
        wp, wb, _keep = knn_workspace(dev, 1, m, m, k + 1)
        call("geot_knn_sorted_ws", dev, 1, m, m, k + 1, ptr(p), ptr(p), ptr(nbr) + 4 * (k + 1) * at, ptr(dist2), wp, wb)
        at += m
    return nbr


def _kept_or_built(batch, sizes, dev, kind, width, build):
    """The table cache of the set (DeviceScanSet.keep_tables) in front of build(batch, sizes) -> (table (sum M, width), stats
    (B, 4) or None).  Off, or a batch without the host scan ids: build(batch, sizes) and nothing else.  On: the scans of the
    batch that have no kept (scan, kind, width) table are built in ONE build call on a batch of just those, each table is kept
    with an event recorded on the building stream, and the batch's table is the kept tables concatenated (device copies); a
    stream other than the one that built a table waits for its event first."""
    scans, ids = batch["scans"], batch.get("ids")
    if not getattr(scans, "_keep", False) or ids is None:
        return build(batch, sizes)
    ids = [int(i) for i in ids]
    need(len(ids) == len(sizes), "the batch's ids must name one scan per slot")
    kept, stream = scans._tables, torch.cuda.current_stream(dev)
    missing = [s for s, i in enumerate(ids) if (i, kind, width) not in kept and i not in ids[:s]]
    if missing:
        part = {"scans": scans, "sizes": [sizes[s] for s in missing], "ids": [ids[s] for s in missing],
                "scan_ids": _to_device(np.asarray([ids[s] for s in missing], dtype=np.int64), dev)}
        if isinstance(batch.get("points"), (list, tuple)) and len(batch["points"]) == len(sizes):
            part["points"] = [batch["points"][s] for s in missing]
        table, st = build(part, part["sizes"])
        event = torch.cuda.Event()
        event.record(stream)
        for j, (s, rows) in enumerate(zip(missing, torch.split(table, part["sizes"]))):
            kept[(ids[s], kind, width)] = (rows, None if st is None else st[j], event, stream)
    tables, rows_st = [], []
    for i in ids:
        rows, st, event, built_on = kept[(i, kind, width)]
        if built_on != stream:
            stream.wait_event(event)
            rows.record_stream(stream)
        tables.append(rows)
        rows_st.append(st)
    return torch.cat(tables), (None if rows_st[0] is None else torch.stack(rows_st))


@torch.no_grad()
def mesh_neighbours(batch, k=MESH_K, stats=False):
    """The one-ring neighbour table of the batch's whole scans from the set's triangles (DeviceScanSet(faces=)): (sum M, k) int32
    on the device, slot after slot -- per vertex the distinct vertices it shares a face with, as indices local to the scan in
    ascending order, the k lowest when there are more, -1 in every unused entry.  The surface's own graph: two teeth in contact
    are not joined by it, as they are by scan_neighbours' Euclidean table, and it needs no search.  One geot_mesh_neighbours
    call (seven launches), no host synchronisation; clean_scans and scan_components take the table as nbr= (or build it
    themselves: mesh=).  stats=True: also the (B, 4) int32 device tensor of usable faces, ignored faces (an index outside the
    scan), truncated vertices (more than k neighbours) and the longest row per scan.
    k: an int in 1..32.  The default 16 rests on no measurement: the mean valence of a closed triangle mesh is 6, but no
    Teeth3DS mesh has been looked at here -- stats[:, 2], the truncated vertices, says whether k is enough for yours.
    The batch must carry the host scan ids ("ids": the whole-scan batchers add them for a set with faces; the face counts are
    the host's).
    ValueError, before any device call, when the set holds no faces or a scan of the batch has no mesh (has_mesh False).
    After scans.keep_tables() every scan's table (and its stats row) is kept on the set and a scan met again costs a device
    copy (DeviceScanSet.keep_tables: the same bits, 4 k M_i bytes per scan)."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= ISLANDS_MAX_K:
        raise ValueError("mesh_neighbours: k must be an int in 1..%d, got %r" % (ISLANDS_MAX_K, k))
    scans, sizes, b, dev = _islands_batch(None, batch, "mesh_neighbours")
    if getattr(scans, "faces", None) is None:
        raise ValueError("mesh_neighbours: the scan set holds no faces -- build it with DeviceScanSet(..., faces=)")
    if batch.get("ids") is None or len(batch["ids"]) != b:
        raise ValueError("mesh_neighbours: the batch must carry its %d scan numbers as host values (\"ids\", as ValBatcher.batch "
                         "adds them): the face counts are the host's" % b)
    ids = [int(i) for i in batch["ids"]]
    for slot, i in enumerate(ids):
        if not 0 <= i < len(scans) or not scans.has_mesh[i]:
            raise ValueError("mesh_neighbours: batch slot %d (scan %d) has no mesh in this set" % (slot, i))
    table, st = _kept_or_built(batch, sizes, dev, "mesh", int(k), lambda part, part_sizes: _mesh_tables(part, part_sizes, dev, int(k)))
    return (table, st) if stats else table


def _mesh_tables(batch, sizes, dev, k):
    """One geot_mesh_neighbours call -> (table, stats)."""
    scans, b, total_out = batch["scans"], len(sizes), sum(sizes)
    counts = [scans.face_sizes[int(i)] for i in batch["ids"]]
    batch_faces = sum(counts)
    nbytes = int(_lib.load().geot_mesh_neighbours_ws_bytes(b, total_out, batch_faces))
    need(nbytes >= 0, "geot_mesh_neighbours: no workspace for b = %d, %d vertices, %d faces" % (b, total_out, batch_faces))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    nbr = torch.empty((total_out, k), dtype=torch.int32, device=dev)
    st = torch.empty((b, 4), dtype=torch.int32, device=dev)
    face_out = _to_device(np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int64), dev)
    call("geot_mesh_neighbours", dev, b, k, len(scans), int(scans.points.shape[0]), int(scans.faces.shape[0]), ptr(scans.faces),
         ptr(scans.offsets), ptr(scans.face_offsets), ptr(batch["scan_ids"].contiguous()), ptr(_out_offsets(sizes, dev)), ptr(face_out),
         batch_faces, ptr(nbr), ptr(st), ptr(ws), nbytes)
    return nbr, st


def _scan_islands(flat, nbr, c, min_size, keep, allowed, batch, sizes, b, dev, want_comp, want_stats):
    """One geot_scan_islands call on the flat int64 label buffer; keep / allowed: host uint32 arrays or None."""
    scans = batch["scans"]
    need(torch.is_tensor(nbr) and nbr.device == dev and nbr.dtype == torch.int32 and nbr.dim() == 2 and nbr.is_contiguous() and
         nbr.shape[0] == sum(sizes) and 1 <= nbr.shape[1] <= ISLANDS_MAX_K,
         "geot_scan_islands: nbr must be a contiguous (%d, 1..%d) int32 tensor on %s" % (sum(sizes), ISLANDS_MAX_K, dev))
    keep = _to_device(keep.view(np.int32), dev) if keep is not None else None
    allowed = _to_device(allowed.view(np.int32), dev) if allowed is not None else None
    nbytes = int(_lib.load().geot_scan_islands_ws_bytes(b, int(flat.numel()), c))
    need(nbytes >= 0, "geot_scan_islands: no workspace for b = %d, c = %d, %d labels" % (b, c, flat.numel()))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    comp = torch.empty(flat.numel(), dtype=torch.int32, device=dev) if want_comp else None
    stats = torch.empty((b, 4), dtype=torch.int32, device=dev) if want_stats else None
    call("geot_scan_islands", dev, b, c, int(nbr.shape[1]), min(min_size, MAX_VERTICES), len(scans), int(scans.points.shape[0]), ptr(scans.offsets),
         ptr(batch["scan_ids"].contiguous()), ptr(_out_offsets(sizes, dev)), ptr(nbr), ptr(keep), ptr(allowed), ptr(flat), ptr(comp),
         ptr(stats), ptr(ws), nbytes)
    return comp, stats


@torch.no_grad()
def scan_components(preds, batch, nbr=None, k=8, num_classes=None, stats=False, mesh=None):
    """The connected pieces of whole-scan labels: per scan of the batch a (1, M_i) int32 tensor (views of one buffer) that
    holds for every vertex the lowest vertex index of its piece -- the vertices of equal label it reaches through the
    neighbour table.  preds as predict_scans and its kin return them; they are not touched.  nbr: scan_neighbours' table, or
    any (sum M, 1..32) int32 table of scan-local indices (default: scan_neighbours(batch, k)).  A label outside [0, C) is a
    piece of its own.  num_classes: default 32.  stats=True: also the (B, 4) int32 device tensor of geot_scan_islands (pieces
    among the labels in [0, C), then three zeros).  mesh (None / False: off): True or an int in 1..32 -- the table is
    mesh_neighbours(batch, 16 or that width), the scan's own triangles; k is then ignored, and nbr with it is a RuntimeError.
    One geot_scan_islands call in its components-only form (four launches), no host synchronisation."""
    width = _mesh_width(mesh, "scan_components")
    need(width is None or nbr is None, "scan_components: mesh and nbr are two tables -- give one")
    scans, sizes, b, dev = _islands_batch(preds, batch, "scan_components")
    c = _need_classes(32 if num_classes is None else num_classes, "scan_components")
    if nbr is None:
        nbr = scan_neighbours(batch, k) if width is None else mesh_neighbours(batch, width)
    flat, _ = _flat_labels(preds, sizes, dev)
    comp, st = _scan_islands(flat, nbr, c, 0, None, None, batch, sizes, b, dev, True, stats)
    out = [q.view(1, -1) for q in torch.split(comp, sizes)]
    return (out, st) if stats else out


@torch.no_grad()
def clean_scans(preds, batch, min_size=10, keep_largest=True, parts=None, nbr=None, k=8, stats=False, num_classes=None, mesh=None):
    """One FDI class in one jaw is one tooth, one connected patch of the surface: preds as predict_scans / vote_scans /
    cover_scans / decode_scans return them -- per scan of the batch a (1, M_i) int64 tensor -- cleaned IN PLACE when they are
    views of one buffer, slot after slot (a list that is not is concatenated and split again); returns the list, with
    stats=True (list, (B, 4) int32 device tensor of pieces, islands, changed vertices, vertices of stranded islands per scan).
    Per scan the labels fall into connected pieces over the neighbour table (scan_components).  A piece is an island when it
    has fewer than min_size vertices, when parts does not allow its class for the scan's jaw, or when its class is kept to one
    piece and it is not the largest (the lowest first vertex among equals); every island takes the label most of its
    vertices' neighbours carry, counting only neighbours of another class that are in no island (the lowest label among
    equals), and stays as it is when there is none.  One pass on the labels as they came in.
    keep_largest: True -- every class from 1 up; class 0, the gingiva, may lie in pieces and is never kept to one -- or an
    iterable of classes, or False.  parts: None or the reference's cls2parts, as for refine_scans.  nbr, k: as for
    scan_components.  num_classes: default parts[-1][-1] + 1, 32 without parts.  mesh: as for scan_components -- "connected"
    then means connected over the scan's triangles (a set built with faces=), not over the 8 nearest vertices in space, which
    join two teeth in contact.  One geot_scan_islands call (six launches) behind the table's searches or its
    geot_mesh_neighbours call, no host synchronisation."""
    min_size, keep, k = _clean_args(min_size, keep_largest, k, "clean_scans")
    width = _mesh_width(mesh, "clean_scans")
    need(width is None or nbr is None, "clean_scans: mesh and nbr are two tables -- give one")
    scans, sizes, b, dev = _islands_batch(preds, batch, "clean_scans")
    if num_classes is None:
        num_classes = 32 if parts is None else int(parts[-1][-1]) + 1
    c = _need_classes(num_classes, "clean_scans")
    allowed = None
    if parts is not None:
        need("mandible" in batch and len(batch["mandible"]) == b, "clean_scans: parts needs the batch's jaw flags (mandible)")
        allowed = _allowed_masks(parts, [0 if m else 1 for m in batch["mandible"]], c, "clean_scans")
    classes = range(1, c) if keep is True else () if keep is False else keep
    need(all(i < c for i in classes), "clean_scans: keep_largest must name classes in [0, %d)" % c)
    mask = sum(1 << i for i in classes)
    keep_masks = np.full(b, mask, dtype=np.uint32) if mask else None
    if nbr is None:
        nbr = scan_neighbours(batch, k) if width is None else mesh_neighbours(batch, width)
    flat, views = _flat_labels(preds, sizes, dev)
    out = list(preds) if views else [f.view(p.shape) for f, p in zip(torch.split(flat, sizes), preds)]
    _, st = _scan_islands(flat, nbr, c, min_size, keep_masks, allowed, batch, sizes, b, dev, False, stats)
    return (out, st) if stats else out


def _finish_labels(preds, batch, n_refine, parts, islands, c):
    """The tail of every label-returning call: refine_scans when refine is on, then clean_scans when islands is."""
    if n_refine:
        preds = refine_scans(preds, batch, n_refine, parts, num_classes=c)
    if islands is not None:
        preds = clean_scans(preds, batch, **dict({"num_classes": c}, **islands))
    return preds


FDI_FIRST = {"lower": (31, 41), "upper": (11, 21)}      # the FDI number of classes 1 and 9 per jaw (the dataset's label2id, inverted)


def teeth3ds_result(labels, comp, jaw, patient=None):
    """The 3DTeethSeg challenge's result dict of one scan, on the host: {"id_patient", "jaw", "labels", "instances"}.
    labels (M,) the scan's classes 0 .. 16 and comp (M,) scan_components' output ON THOSE LABELS (after clean_scans), as
    tensors (one device-to-host copy for both) or arrays; jaw "lower" or "upper".  "labels" are FDI numbers, the inverse of
    the dataset's label2id for that jaw -- lower: 1..8 -> 31..38, 9..16 -> 41..48; upper: 1..8 -> 11..18, 9..16 -> 21..28;
    0 -> 0 -- and "instances" is 0 for the gingiva and 1, 2, ... for the connected pieces of teeth by ascending first vertex:
    a class that lies in two pieces is two instances.  Both are lists of M ints."""
    if jaw not in FDI_FIRST:
        raise ValueError("teeth3ds_result: jaw must be 'lower' or 'upper', got %r" % (jaw,))
    if torch.is_tensor(labels) and torch.is_tensor(comp):
        need(labels.numel() == comp.numel(), "teeth3ds_result: %d labels and %d components" % (labels.numel(), comp.numel()))
        both = torch.stack([labels.reshape(-1).to(torch.int64), comp.reshape(-1).to(torch.int64)]).cpu().numpy()
        lab, cmp_ = both[0], both[1]
    else:
        lab = np.asarray(labels.cpu() if torch.is_tensor(labels) else labels).reshape(-1).astype(np.int64)
        cmp_ = np.asarray(comp.cpu() if torch.is_tensor(comp) else comp).reshape(-1).astype(np.int64)
        need(lab.size == cmp_.size, "teeth3ds_result: %d labels and %d components" % (lab.size, cmp_.size))
    need(lab.size == 0 or (lab.min() >= 0 and lab.max() <= 16), "teeth3ds_result: labels must lie in 0 .. 16")
    first, second = FDI_FIRST[jaw]
    fdi = np.where(lab == 0, 0, np.where(lab <= 8, first - 1 + lab, second - 9 + lab))
    tooth = lab > 0
    roots = np.unique(cmp_[tooth])                      # ascending
    instances = np.zeros(lab.size, dtype=np.int64)
    instances[tooth] = np.searchsorted(roots, cmp_[tooth]) + 1
    return {"id_patient": patient, "jaw": jaw, "labels": fdi.tolist(), "instances": instances.tolist()}


def _mandible_flags(cls, b):
    """validate's `cls[ii] == 0` for the b scans of a batch, on the host (a device tensor costs one copy here)."""
    if torch.is_tensor(cls):
        cls = cls.detach().cpu()
    need(len(cls) == b, "SegMetrics: %d jaw classes (cls) for %d scans" % (len(cls), b))
    return [bool(cls[i] == 0) for i in range(b)]


class SegMetrics:
    """The validation metrics of one epoch, counted on the device: a (scans, C (C + 1) + 1) int64 buffer (its capacity
    doubles as scans arrive) and each scan's jaw, kept on the host.  Neither update synchronises with the host."""

    def __init__(self, num_classes, device):
        c = _need_classes(num_classes, "SegMetrics")
        dev = torch.device(device)
        need(dev.type == "cuda", "SegMetrics: the counts live on a GPU, got device %s" % dev)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.c, self.slots, self.device = c, c * (c + 1) + 1, dev
        self.counts = torch.zeros((8, self.slots), dtype=torch.int64, device=dev)
        self.mandible = []

    @property
    def scans(self):
        return len(self.mandible)

    def reset(self):
        """A new epoch."""
        self.counts.zero_()
        self.mandible = []

    def _rows(self, b):
        """The (zero) count rows of the next b scans."""
        n0 = self.scans
        if n0 + b > self.counts.shape[0]:
            grown = torch.zeros((max(n0 + b, 2 * self.counts.shape[0]), self.slots), dtype=torch.int64, device=self.device)
            grown[:n0].copy_(self.counts[:n0])
            self.counts = grown
        return self.counts[n0:n0 + b]

    def _offsets(self, sizes):
        """(b + 1) int64 on the device; the caller keeps the tensor until its launch is queued."""
        for m in sizes:
            need(m <= MAX_VERTICES, "SegMetrics: %d vertices in one scan, at most %d" % (m, MAX_VERTICES))
        offs = torch.tensor(np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]), dtype=torch.int64)
        return offs.pin_memory().to(self.device, non_blocking=True)      # no synchronisation

    def _labels(self, labels_whole):
        labels = [torch.as_tensor(l).reshape(-1) for l in labels_whole]
        need(all(not l.is_floating_point() for l in labels), "SegMetrics: integer labels")
        return torch.cat([l.to(self.device, torch.int64) for l in labels]), [l.numel() for l in labels]

    def update(self, preds_whole, labels_whole, cls):
        """Count one batch from predictions: preds_whole / labels_whole lists of the b scans' per-vertex predictions (e.g.
        get_pred_whole's (1, M_i)) and labels (M_i,); cls the b jaw classes (0 = mandible), as the loader hands them over."""
        b = len(preds_whole)
        need(len(labels_whole) == b, "SegMetrics.update: %d prediction and %d label tensors" % (b, len(labels_whole)))
        flags = _mandible_flags(cls, b)
        if b == 0:
            return
        preds = [torch.as_tensor(p).reshape(-1) for p in preds_whole]
        need(all(not p.is_floating_point() for p in preds), "SegMetrics.update: integer predictions")
        label, sizes = self._labels(labels_whole)
        need([p.numel() for p in preds] == sizes, "SegMetrics.update: every scan needs one prediction per vertex")
        rows = self._rows(b)
        if sum(sizes):
            pred = torch.cat([p.to(self.device, torch.int64) for p in preds])
            offs = self._offsets(sizes)
            call("geot_seg_confusion", self.device, b, self.c, ptr(offs), ptr(pred), ptr(label), ptr(rows))
        self.mandible += flags

    def update_from_logits(self, logits, points, points_whole, center, scale, labels_whole, cls):
        """Count one batch from the model's logits (B, C, N) with get_pred_whole's arguments (points (B, N, 3) normalised,
        points_whole / center / scale per scan) plus the scans' labels and jaw classes: get_pred_whole's soft-max,
        de-normalisation and three_nn, then one launch that interpolates, arg-maxes and counts."""
        need(torch.is_tensor(logits) and logits.dim() == 3 and logits.shape[1] == self.c and logits.dtype == torch.float32,
             "SegMetrics.update_from_logits: fp32 logits (B, %d, N)" % self.c)
        need(logits.device == self.device, "SegMetrics.update_from_logits: logits on %s, the counts on %s" %
             (logits.device, self.device))
        b, _, n = logits.shape
        need(len(points_whole) == b and len(center) == b and len(scale) == b and len(labels_whole) == b,
             "SegMetrics.update_from_logits: one points_whole / center / scale / labels entry per scan")
        need(tuple(points.shape) == (b, n, 3), "SegMetrics.update_from_logits: points must be (B, N, 3)")
        flags = _mandible_flags(cls, b)
        if b == 0:
            return
        dev = self.device
        prob = F.softmax(logits, dim=1).contiguous()
        label, sizes = self._labels(labels_whole)
        total = sum(sizes)
        idx = torch.empty((total, 3), dtype=torch.int32, device=dev)
        dist2 = torch.empty((total, 3), dtype=torch.float32, device=dev)
        at = 0
        for index in range(b):
            # get_pred_whole's three_nn inputs, statement for statement; its output goes into this scan's slice
            unknown, known = _three_nn_inputs(points, points_whole, center, scale, index, dev)
            m = unknown.shape[1]
            need(unknown.dim() == 3 and unknown.shape[2] == 3 and m == sizes[index],
                 "SegMetrics.update_from_logits: scan %d has %d labels for %s vertices" % (index, sizes[index],
                                                                                           tuple(unknown.shape[1:])))
            if m:
                wp, wb, _keep = knn_workspace(dev, 1, m, n, 3)
                call("geot_three_nn_ws", dev, 1, m, n, ptr(unknown), ptr(known), ptr(dist2) + 12 * at, ptr(idx) + 12 * at,
                     wp, wb)
            at += m
        rows = self._rows(b)
        if total:
            offs = self._offsets(sizes)
            call("geot_seg_confusion_interp", dev, b, self.c, n, ptr(offs), ptr(prob), ptr(idx), ptr(dist2), ptr(label),
                 ptr(rows))
        self.mandible += flags

    def _scan_rows(self, batch, what):
        """The jaw flags of a ValBatcher / VoteBatcher batch and the count rows of its scans."""
        need(isinstance(batch, dict) and "mandible" in batch, "SegMetrics.%s: batch must come from ValBatcher.batch" % what)
        need(batch["scans"].device == self.device, "SegMetrics.%s: the scans on %s, the counts on %s" %
             (what, batch["scans"].device, self.device))
        flags = [bool(m) for m in batch["mandible"]]
        need(len(flags) == len(batch["sizes"]), "SegMetrics.%s: one jaw flag per scan" % what)
        return flags, self._rows(len(flags))

    def update_from_scans(self, logits, batch, want_pred=False):
        """Count one ValBatcher batch from the model's logits (B, C, N): update_from_logits' counts, from the scans where
        they lie -- one geot_scan_predict call whatever B and the scans' sizes, the jaws from the batch's host flags, no
        host synchronisation.  want_pred: the same call also writes the labels -> as predict_scans returns them."""
        flags, rows = self._scan_rows(batch, "update_from_scans")
        preds = _scan_launch(logits, batch, self.c, "SegMetrics.update_from_scans", counts=rows, want_pred=want_pred)
        self.mandible += flags
        return preds

    def update_from_votes(self, votes, logits, batch, want_pred=False):
        """Count one batch of scans from its votes: `votes` (a ScanVotes of C classes) holds the earlier passes, the model's
        logits on `batch` are the last one -- votes.add(logits, batch, last=True) with this epoch's next rows as counts, one
        geot_scan_vote call; the jaws from the batch's host flags, no host synchronisation.  want_pred: the same call also
        writes the voted labels -> as vote_scans returns them."""
        need(votes.c == self.c, "SegMetrics.update_from_votes: the votes have %d classes, the counts %d" % (votes.c, self.c))
        flags, rows = self._scan_rows(batch, "update_from_votes")
        preds = votes.add(logits, batch, last=True, counts=rows, want_pred=want_pred)
        self.mandible += flags
        return preds

    def read(self):
        """The epoch so far, in one device-to-host copy: per scan "acc_list" (0-d fp32 tensors), "miou_list" / "mdsc_list"
        (numpy scalars: float32, or a float64 NaN for a scan with no label but 0), as get_seg_metrics returns them; per jaw
        and whole "mandible_macc" ... "whole_mdsc" as validate computes them; "scans", "labels_out_of_range".  Raises
        RuntimeError if a label outside [0, C) was seen."""
        return seg_metrics_from_counts(self.counts[:self.scans].cpu().numpy(), self.c, self.mandible)


@torch.no_grad()
def get_seg_metrics(preds_whole, labels_whole, num_classes=17):
    """train.py:802-832: (acc_list, miou_list, mdsc_list) of the scans, the reference's values and types."""
    p0 = preds_whole[0] if len(preds_whole) else None
    dev = p0.device if torch.is_tensor(p0) and p0.is_cuda else torch.device("cuda", torch.cuda.current_device())
    metrics = SegMetrics(num_classes, dev)
    metrics.update(preds_whole, labels_whole, [0] * len(preds_whole))
    out = metrics.read()
    return out["acc_list"], out["miou_list"], out["mdsc_list"]


def _cfg(cfg, key, default=None):
    return getattr(cfg, key) if hasattr(cfg, key) else (cfg.get(key, default) if hasattr(cfg, "get") else default)


@torch.no_grad()
def validate(model, val_loader, cfg, num_votes=0, data_transform=None):
    """train.py:716-779 over collate_fn_val batches (openpoints/dataset/build.py:30-50) -> (whole_macc, whole_miou,
    whole_mdsc), logging the reference's three lines.  cfg.num_classes (default 17) sizes the counts.  num_votes and
    data_transform are accepted and unused, as in the reference."""
    model.eval()
    metrics = SegMetrics(_cfg(cfg, "num_classes", 17), torch.device("cuda", torch.cuda.current_device()))
    for data in val_loader:
        cls = data["cls"]                  # the loader's CPU tensor: each scan's jaw, read before anything moves
        for key in data.keys():
            if isinstance(data[key], torch.Tensor):
                data[key] = data[key].cuda(non_blocking=True)
        data["x"] = data["x"].transpose(1, 2).contiguous()
        logits, _, _ = model(data)
        metrics.update_from_logits(logits, data["pos"], data["points"], data["center"], data["scale"], data["labels"], cls)
    return _report(metrics.read(), cfg)


def _report(out, cfg):
    """validate's three log lines and its return value."""
    epoch = "%s/%s" % (_cfg(cfg, "epoch"), _cfg(cfg, "epochs"))
    with np.printoptions(precision=2, suppress=True):
        logging.info(f"Test Epoch [{epoch}],Mandible mIoU {out['mandible_miou']:.5f}, "
                     f"Mandible DSC {out['mandible_mdsc']:.5f}, Mandible ACC {out['mandible_macc']:.5f}")
        logging.info(f"Test Epoch [{epoch}],Maxillary mIoU {out['maxillary_miou']:.5f}, "
                     f"Maxillary DSC {out['maxillary_mdsc']:.5f}, Maxillary ACC {out['maxillary_macc']:.5f}")
        logging.info(f"Test Epoch [{epoch}],mIoU {out['whole_miou']:.5f}, DSC {out['whole_mdsc']:.5f}, "
                     f"ACC {out['whole_macc']:.5f}")
    return out["whole_macc"], out["whole_miou"], out["whole_mdsc"]


def _replay_switches(graph, lookahead, num_votes, model, what):
    """The `graph` / `lookahead` keywords of validate_scans, validate_scans_voted and vote_scans, checked before any device
    call -> (G, the GraphedForward or None).  lookahead: False / 0 (off), True (G = max(num_votes, 1): a voted group's passes
    share one geometry call) or an int G >= 1; graph: False, True (the model's own wrapper, graph_eval.graphed_forward) or a
    GraphedForward built on the model; graph without lookahead runs at G = 1 (a replay needs a static geometry).  TypeError
    for another type (a bool is no int: graph=1 is refused like lookahead=2.0), ValueError for G < 0 or
    G > graph_eval.MAX_LOOKAHEAD."""
    if not isinstance(graph, (bool, graph_eval.GraphedForward)):
        raise TypeError("%s: graph must be a bool or a GraphedForward, got %r" % (what, graph))
    if isinstance(lookahead, bool):
        g = max(int(num_votes), 1) if lookahead else 0
    elif isinstance(lookahead, (int, np.integer)):
        g = int(lookahead)
    else:
        raise TypeError("%s: lookahead must be a bool or an int, got %r" % (what, lookahead))
    if g < 0:
        raise ValueError("%s: lookahead must be >= 0, got %r" % (what, lookahead))
    if graph is not False:
        g = max(g, 1)
    if g > graph_eval.MAX_LOOKAHEAD:
        raise ValueError("%s: at most %d passes are drawn ahead, got lookahead = %d" % (what, graph_eval.MAX_LOOKAHEAD, g))
    if isinstance(graph, graph_eval.GraphedForward) and graph.model is not model:
        raise ValueError("%s: the GraphedForward was built on another model" % what)
    return g, graph if isinstance(graph, graph_eval.GraphedForward) else graph_eval.graphed_forward(model) if graph else None


def pass_schedule(group_sizes, repeats, lookahead):
    """The order of a whole-scan run as pure host logic: groups of group_sizes scans, each `repeats` passes, G = lookahead
    passes drawn ahead -> (passes, ops); passes: (group number, first pass of its group, last pass of its group); ops in
    execution order: ("draw", k) -- batcher.batch() for pass k, ALWAYS in pass order, so the host generators and the DeviceDraws
    counters see today's sequence of calls, only earlier; ("geometry", (k, ...)) -- one prefetch_geometry over these passes'
    positions concatenated; ("forward", k).  The passes are cut into chunks of G.  A chunk is drawn at once, and its passes with
    a full batch (as many scans as the largest group) share one geometry call; a shorter batch is left out and computes its
    geometry in line.  The first chunk is announced before anything runs; every other one in front of the forward pass of
    the last pass before it, beside which its geometry runs."""
    repeats, g = int(repeats), int(lookahead)
    need(g >= 1, "pass_schedule: lookahead >= 1 (without it _passes runs its own loop)")
    passes = [(group, k == 0, k + 1 == repeats) for group in range(len(group_sizes)) for k in range(repeats)]
    n, ops = len(passes), []
    if not n:
        return passes, ops
    full = max(int(s) for s in group_sizes)

    def chunk(start):
        members = range(start, min(start + g, n))
        ops.extend(("draw", k) for k in members)
        shared = tuple(k for k in members if int(group_sizes[passes[k][0]]) == full)
        if shared:
            ops.append(("geometry", shared))
    chunk(0)
    for k in range(n):
        if (k + 1) % g == 0 and k + 1 < n:
            chunk(k + 1)
        ops.append(("forward", k))
    return passes, ops


class _Shared:
    """One concatenated geometry (None: the model has none to give) and the positions it was computed from: pass `index` takes
    its slice only for the very tensor that was concatenated, unedited -- a static geometry has no identities of its own, so
    this is where they are checked.  ready: the event behind the work, when a side stream did it."""

    def __init__(self, geometry, positions, ready=None):
        self.geometry, self.ready = geometry, ready
        self.sources = [(p, p._version) for p in positions]
        self.rows = np.concatenate([[0], np.cumsum([int(p.shape[0]) for p in positions])]).tolist()

    def slice_for(self, index, pos):
        src, version = self.sources[index]
        if self.geometry is None or src is not pos or pos._version != version:
            return None
        return self.geometry.slice(self.rows[index], self.rows[index + 1])


_AHEAD_STREAMS = {}     # device -> the stream the eager look-ahead geometry runs on


class _EagerAhead:
    """The look-ahead of _passes on eager launches: the concatenated geometry on a side stream of its own (the model's side
    stream is waited for by every forward pass that computes its geometry in line), as a static Geometry this object vouches
    for; the forward pass waits for its event."""

    def __init__(self, model):
        self.model = model

    def start(self, batches):
        positions = [b["pos"] for b in batches]
        dev = positions[0].device
        seg = getattr(self.model, "segmentor", self.model)
        if not (hasattr(self.model, "prefetch_geometry") and positions[0].is_cuda and getattr(seg, "overlap", True)
                and streams.may_fork(dev)):
            return _Shared(None, positions)
        main = torch.cuda.current_stream(dev)
        if dev not in _AHEAD_STREAMS:
            _AHEAD_STREAMS[dev] = torch.cuda.Stream(device=dev)
        side = _AHEAD_STREAMS[dev]
        cat = positions[0] if len(positions) == 1 else torch.cat(positions, 0)
        side.wait_stream(main)              # the batches are joined, the concatenation is queued: beside what follows on main
        with torch.cuda.stream(side):
            geometry = self.model.prefetch_geometry(cat, inline=True)
            ready = streams.event()
            ready.record(side)
        cat.record_stream(side)
        for _, t in graph_eval.tree_tensors(geometry):      # side-stream memory the current stream will read
            t.record_stream(main)
        return _Shared(geometry, positions, ready)

    def forward(self, data, share, next_batches):
        token = self.start(next_batches) if next_batches else None
        geometry = None
        if share is not None:
            shared, index = share
            if shared.ready is not None:
                torch.cuda.current_stream(data["pos"].device).wait_event(shared.ready)
            geometry = shared.slice_for(index, data["pos"])
        out = self.model(data) if geometry is None else self.model(data, geometry=geometry)
        return out[0], token


class _GraphedAhead:
    """The look-ahead of _passes on a graph_eval.GraphedForward: P on its side stream, F replayed over the pass's slice."""

    def __init__(self, graphed):
        self.graphed = graphed

    def start(self, batches):
        positions = [b["pos"] for b in batches]
        return _Shared(self.graphed.lookahead(positions), positions)

    def forward(self, data, share, next_batches):
        geometry = None
        if share is not None:
            self.graphed.join()             # the slice below reads P's product
            geometry = share[0].slice_for(share[1], data["pos"])
        positions = [b["pos"] for b in next_batches] if next_batches else None
        out = self.graphed(data, geometry, next_positions=positions)
        return out[0], _Shared(self.graphed.ahead, positions) if positions else None


def _passes(model, batcher, groups, repeats, draws, lookahead=0, graphed=None, runner=None, feed=None):
    """The look-ahead loop of every whole-scan pass: each list of scan numbers in `groups` runs through the model `repeats`
    times, each time on a freshly drawn batch -> (batch, logits, first pass of its group, last pass of its group) per pass.
    The next pass's batch is queued BEFORE the current forward pass -- beside it when the batcher has a side stream -- and
    the host draws (np.random.choice) happen inside batch(): seeded runs are equal only while this order holds.  draws goes to
    every batch() call as it is.
    lookahead = G >= 1 (pass_schedule): up to G passes are drawn ahead -- the same batch() calls in the same order -- and
    their coordinate-only work (Group, the largest FPS, the index plan) runs as ONE prefetch_geometry over their concatenated
    positions beside the forward pass in flight; each pass takes its Geometry.slice.  graphed: a graph_eval.GraphedForward
    -- that geometry call and every forward pass replay from hipGraphs, and the logits of a pass are a fixed buffer the next
    pass overwrites (a consumer uses them before it asks for the next pass).  runner: the object that does both (tests).
    feed: a callable k -> the batch of pass k, asked in pass order, in place of batcher.batch() (the covering passes)."""
    passes = [(ids, k == 0, k + 1 == repeats) for ids in groups for k in range(repeats)]
    if feed is None:
        def feed(k):
            return batcher.batch(passes[k][0], draws=draws)
    if not lookahead:
        data = feed(0) if passes else None
        for k, (_, first, last) in enumerate(passes):
            batcher.join(data)
            ahead = feed(k + 1) if k + 1 < len(passes) else None
            logits, _, _ = model(data)
            yield data, logits, first, last
            data = ahead
        return
    if runner is None:
        runner = _GraphedAhead(graphed) if graphed is not None else _EagerAhead(model)
    batches, shares, joined, announced, ran = {}, {}, set(), None, False

    def join(k):
        if k not in joined:
            batcher.join(batches[k])
            joined.add(k)
    for op, arg in pass_schedule([len(ids) for ids in groups], repeats, lookahead)[1]:
        if op == "draw":
            batches[arg] = feed(arg)
        elif op == "geometry":
            for j in arg:
                join(j)
            if not ran:                     # the first chunk: no forward pass is in flight to run beside
                token = runner.start([batches[j] for j in arg])
                shares.update((j, (token, i)) for i, j in enumerate(arg))
                ran = True
            else:                           # started by the forward pass that follows, beside it
                announced = arg
        else:
            upcoming, announced, ran = announced, None, True
            join(arg)
            data = batches.pop(arg)
            joined.discard(arg)
            logits, token = runner.forward(data, shares.pop(arg, None), [batches[j] for j in upcoming] if upcoming else None)
            if upcoming:
                shares.update((j, (token, i)) for i, j in enumerate(upcoming))
            yield (data, logits) + passes[arg][1:]


def _validate(model, batcher, cfg, c, batch_size, indices, num_votes, draws, n_refine, parts, what, lookahead=0, graphed=None,
              teeth=None, islands=None):
    """The body of validate_scans (num_votes = 0: one pass per batch, scored by geot_scan_predict) and validate_scans_voted
    (num_votes passes per batch, summed by geot_scan_vote and scored on the last): batches of batch_size scans in `indices`'
    order through _passes, counted into one SegMetrics; with n_refine the labels are taken, refined and counted instead.
    teeth (a ToothScores): the call that counts also writes the labels, and every batch's final labels go through teeth.update.
    islands (_islands_kw's dict or None): as n_refine, the labels are taken, cleaned behind the refinement and counted."""
    need(int(batch_size) >= 1, "%s: batch_size >= 1" % what)
    _need_teeth(teeth, c, batcher.device, what)
    order = list(range(len(batcher))) if indices is None else [int(i) for i in indices]
    groups = [order[at:at + int(batch_size)] for at in range(0, len(order), int(batch_size))]
    metrics = SegMetrics(c, batcher.device)
    votes = None
    for data, logits, first, last in _passes(model, batcher, groups, max(num_votes, 1), draws, lookahead, graphed):
        if num_votes and first:
            votes = ScanVotes(data, c)
        if not last:
            votes.add(logits, data)
        elif n_refine or islands is not None:
            preds = (votes.add(logits, data, last=True, want_pred=True) if num_votes else
                     _scan_launch(logits, data, c, what, want_pred=True))
            preds = _count_refined(metrics, preds, data, n_refine, parts, islands)
        elif num_votes:
            preds = metrics.update_from_votes(votes, logits, data, want_pred=teeth is not None)
        else:
            preds = metrics.update_from_scans(logits, data, want_pred=teeth is not None)
        if last and teeth is not None:
            teeth.update(preds, data)
    return _report(metrics.read(), cfg)


@torch.no_grad()
def validate_scans(model, scans, cfg, batch_size=2, indices=None, stream=None, num_votes=0, data_transform=None, refine=0,
                   parts=None, graph=False, lookahead=0, teeth=None, islands=None):
    """validate() without a loader: scans a DeviceScanSet (or a ValBatcher built on one, reused from epoch to epoch),
    batches of batch_size scans in the sequential sampler's order (the last, shorter batch is kept: drop_last is false for
    `val`), or of the scans `indices` names (a rank's shard).  cfg.num_points sizes the sample, cfg.num_classes (default
    17) the counts.  Same log lines, return value and dtypes as validate().  stream: the next batch is built on that side
    stream while the current one runs through the model.  num_votes and data_transform are accepted and unused, as in the
    reference.  refine (0: off -- cfg.refine is not read; True: n = 10; an int: n) and parts: the per-vertex labels are taken,
    refined (refine_scans) and counted against the scans' labels with geot_seg_confusion.  graph, lookahead
    (_replay_switches, _passes): the passes' geometry computed ahead and the forward passes replayed from hipGraphs -- the
    same values; off by default.  teeth: a ToothScores (None: off, and every call is as without the keyword) -- each batch's
    final labels, after refine where that is on, also go through teeth.update; geot_scan_predict then writes the labels in the
    call that counts them.  The return value stays the three-tuple: the caller reads teeth.read().  islands (None / False: off,
    and every call is as without the keyword; True or a dict: predict_scans' keyword): the labels are taken, cleaned
    (clean_scans) behind the refinement, and counted with geot_seg_confusion; teeth sees the cleaned labels."""
    from .openpoints.dataset.val_batch import ValBatcher
    n_refine = _refine_n(refine, "validate_scans")
    islands = _islands_kw(islands, "validate_scans")
    lookahead, graphed = _replay_switches(graph, lookahead, 0, model, "validate_scans")
    model.eval()
    c = _cfg(cfg, "num_classes", 17)
    if isinstance(scans, ValBatcher):
        batcher = scans
        need(stream is None or stream is batcher.stream, "validate_scans: the ValBatcher was built for another stream")
    else:
        need(_cfg(cfg, "num_points") is not None, "validate_scans: cfg.num_points (the sample size) is missing")
        batcher = ValBatcher(scans, _cfg(cfg, "num_points"), c, stream=stream)
    _need_mesh(islands, batcher, "validate_scans")
    return _validate(model, batcher, cfg, c, batch_size, indices, 0, None, n_refine, parts, "validate_scans", lookahead, graphed,
                     teeth, islands)


def _scan_labels(batch):
    """The labels of the batch's scans, gathered from the set on the device: list of (M_i,) int64.  The sizes are the host's,
    the scan ids stay on the device: no synchronisation."""
    scans, sizes = batch["scans"], [int(m) for m in batch["sizes"]]
    dev, b, total = scans.device, len(sizes), sum(sizes)
    reps = _to_device(np.asarray(sizes, dtype=np.int64), dev)
    slot = torch.repeat_interleave(torch.arange(b, device=dev), reps, output_size=total)
    first = scans.offsets[batch["scan_ids"]] - _out_offsets(sizes, dev)
    index = first[slot] + torch.arange(total, device=dev)
    return list(torch.split(scans.labels[index].to(torch.int64), sizes))


def _count_refined(metrics, preds, batch, n, parts, islands=None):
    """The validators' refine / islands leg: refine (n > 0) and clean (islands: _islands_kw's dict) the batch's per-vertex
    labels and count them against the scans' labels -> the final labels."""
    preds = _finish_labels(preds, batch, n, parts, islands, metrics.c)
    metrics.update(preds, _scan_labels(batch), [0 if m else 1 for m in batch["mandible"]])
    return preds


class ScanVotes:
    """The votes of one batch of scans: the accumulator -- fp32 (sum of the scans' vertices, C), vertex-major, slot after slot --
    its out_offsets and the work table, made once; every add() is one geot_scan_vote call.  batch: a VoteBatcher (or
    ValBatcher) batch of the scans voted on; every later batch must name the same scans in the same slots.  Nothing here
    synchronises with the host."""

    def __init__(self, batch, num_classes):
        need(isinstance(batch, dict) and all(k in batch for k in ("scans", "sizes", "scan_ids")),
             "ScanVotes: batch must come from VoteBatcher.batch or ValBatcher.batch")
        c = _need_classes(num_classes, "ScanVotes")
        self.scans, self.sizes, self.c = batch["scans"], [int(m) for m in batch["sizes"]], c
        need(1 <= len(self.sizes) <= SCAN_MAX_SLOTS, "ScanVotes: 1 .. %d scans" % SCAN_MAX_SLOTS)
        dev = self.device = self.scans.device
        self.acc = torch.empty((sum(self.sizes), c), dtype=torch.float32, device=dev)      # the first add() stores
        self.out_offsets = _out_offsets(self.sizes, dev)
        self.work = _to_device(scan_work_table(self.sizes), dev)
        self.votes, self.finished = 0, False

    def add(self, logits, batch, last=False, counts=None, want_pred=False):
        """One vote: the model's logits (B, C, N) on `batch`, a fresh sample of the same scans.  get_pred_whole's soft-max,
        the de-normalisation of batch["pos_search"] (a plain ValBatcher batch: batch["pos"]) and one geot_scan_vote call that
        adds the interpolated probabilities of every vertex.  last: the arg-max of the sums is taken; then counts (rows of a
        SegMetrics buffer, ADDED to) and want_pred (-> list of (1, M_i) int64 labels, as predict_scans returns them) are
        allowed."""
        need(not self.finished, "ScanVotes.add: the last vote has been added")
        need(last or (counts is None and not want_pred), "ScanVotes.add: counts and predictions come with the last vote (last=True)")
        mode = (_lib.VOTE_SET if self.votes == 0 else 0) | (_lib.VOTE_FINISH if last else 0)
        preds = _scan_launch(logits, batch, self.c, "ScanVotes.add", counts, want_pred, votes=self, mode=mode)
        self.votes += 1
        self.finished = bool(last)
        return preds

    def probabilities(self):
        """Per scan the (M_i, C) mean of the votes so far: the accumulator's rows times 1 / votes."""
        need(self.votes >= 1, "ScanVotes.probabilities: no vote yet")
        return list(torch.split(self.acc * (1.0 / self.votes), self.sizes))


@torch.no_grad()
def vote_scans(model, batcher, idx, num_votes, draws=None, refine=0, parts=None, graph=False, lookahead=0, islands=None):
    """The voted per-vertex labels of the scans `idx` of a VoteBatcher's set: list of (1, M_i) int64 tensors, as predict_scans
    returns them.  num_votes model passes, each on a freshly drawn batch of the same scans (draws: a DeviceDraws for these
    batches; default: the batcher's); the next batch is built beside the forward pass when the batcher has a side stream.
    refine (0: off, True: n = 10, an int: n) and parts: the voted labels then go through refine_scans.  graph, lookahead: as
    for validate_scans; lookahead=True runs ONE geometry call for all num_votes passes.  islands: as for predict_scans."""
    need(int(num_votes) >= 1, "vote_scans: num_votes >= 1")
    n_refine = _refine_n(refine, "vote_scans")
    islands = _islands_kw(islands, "vote_scans")
    lookahead, graphed = _replay_switches(graph, lookahead, int(num_votes), model, "vote_scans")
    _need_mesh(islands, batcher, "vote_scans")
    model.eval()
    votes = preds = None
    for data, logits, first, last in _passes(model, batcher, [idx], int(num_votes), draws, lookahead, graphed):
        if first:
            votes = ScanVotes(data, logits.shape[1])
        preds = votes.add(logits, data, last=last, want_pred=last)
    return _finish_labels(preds, data, n_refine, parts, islands, votes.c)


@torch.no_grad()
def validate_scans_voted(model, scans, cfg, num_votes=None, vote=None, batch_size=2, indices=None, stream=None, draws=None,
                         refine=0, parts=None, graph=False, lookahead=0, teeth=None, islands=None):
    """validate_scans with votes: every batch of scans runs through the model num_votes times, each time freshly sampled and
    under the `vote` transform list, and is scored on the arg-max of the summed whole-scan probabilities.  scans: a
    DeviceScanSet, or a VoteBatcher built on one.  num_votes defaults to cfg.num_votes, vote to cfg.datatransforms.vote when
    present (else VoteBatcher's default, the yaml's [PointCloudScaling]); the lists' kwargs to cfg.datatransforms.kwargs.
    num_votes < 1 raises ValueError: validate_scans is the un-voted call.  The next vote's batch is built on `stream` beside
    the current forward pass.  Same log lines, return value and dtypes as validate().  refine, parts: as for validate_scans,
    on the voted labels.  graph, lookahead: as for validate_scans; lookahead=True draws a group's num_votes passes at once
    and runs one geometry call for them.  teeth: as for validate_scans, on the voted labels (the last geot_scan_vote call writes
    them beside the counts).  islands: as for validate_scans, on the voted labels."""
    from .openpoints.dataset.vote_batch import DEFAULT_VOTE, TOOTH_VIEW_KWARGS, VoteBatcher
    n_refine = _refine_n(refine, "validate_scans_voted")
    islands = _islands_kw(islands, "validate_scans_voted")
    num_votes = _cfg(cfg, "num_votes", 0) if num_votes is None else num_votes
    if num_votes is None or int(num_votes) < 1:
        raise ValueError("validate_scans_voted: num_votes must be >= 1, got %r (validate_scans is the un-voted call)" % (num_votes,))
    num_votes = int(num_votes)
    lookahead, graphed = _replay_switches(graph, lookahead, num_votes, model, "validate_scans_voted")
    model.eval()
    c = _cfg(cfg, "num_classes", 17)
    if isinstance(scans, VoteBatcher):
        batcher = scans
        need(stream is None or stream is batcher.stream, "validate_scans_voted: the VoteBatcher was built for another stream")
        need(vote is None or list(vote) == batcher.vote, "validate_scans_voted: the VoteBatcher was built for another vote list")
    else:
        need(_cfg(cfg, "num_points") is not None, "validate_scans_voted: cfg.num_points (the sample size) is missing")
        transforms = _cfg(cfg, "datatransforms")
        if vote is None:
            vote = _cfg(transforms, "vote") if transforms is not None else None
        kwargs = _cfg(transforms, "kwargs") if transforms is not None else None
        batcher = VoteBatcher(scans, _cfg(cfg, "num_points"), c, vote=DEFAULT_VOTE if vote is None else vote,
                              kwargs=TOOTH_VIEW_KWARGS if kwargs is None else kwargs, stream=stream, draws=draws)
    _need_mesh(islands, batcher, "validate_scans_voted")
    return _validate(model, batcher, cfg, c, batch_size, indices, num_votes, draws, n_refine, parts, "validate_scans_voted",
                     lookahead, graphed, teeth, islands)


class ScanCover:
    """The sums of one batch of scans under covering passes (ScanBatcher.cover): ScanVotes' accumulator -- fp32 (sum of the
    scans' vertices, C), vertex-major, slot after slot -- its out_offsets and the work table, made once; every add() is one
    geot_scan_cover call, which puts the model's probabilities for sample j of a pass on the vertex that sample IS: no search, no
    interpolation.  batch: any batch of the scans covered; every later batch must name the same scans in the same slots.
    Nothing here synchronises with the host."""

    def __init__(self, batch, num_classes):
        need(isinstance(batch, dict) and all(k in batch for k in ("scans", "sizes", "scan_ids")),
             "ScanCover: batch must come from a ValBatcher's or VoteBatcher's cover()")
        c = _need_classes(num_classes, "ScanCover")
        self.scans, self.sizes, self.c = batch["scans"], [int(m) for m in batch["sizes"]], c
        need(1 <= len(self.sizes) <= SCAN_MAX_SLOTS, "ScanCover: 1 .. %d scans" % SCAN_MAX_SLOTS)
        dev = self.device = self.scans.device
        self.acc = torch.empty((sum(self.sizes), c), dtype=torch.float32, device=dev)      # round 0 stores
        self.out_offsets = _out_offsets(self.sizes, dev)
        self.work = _to_device(scan_work_table(self.sizes), dev)
        self.rounds, self.finished = 0, False

    def add(self, logits, batch, last=False, counts=None, want_pred=False):
        """One pass: the model's logits (B, C, m) on `batch`, one of cover()'s.  get_pred_whole's soft-max, then one
        geot_scan_cover call: the probabilities of every sample that owns a vertex (batch["sel"], batch["cover"]) are stored in
        (round 0) or added to that vertex's row.  last (legal on the last pass of a round alone): the arg-max of the sums is
        taken; then counts (rows of a SegMetrics buffer, ADDED to) and want_pred (-> list of (1, M_i) int64 labels, as
        predict_scans returns them) are allowed."""
        what = "ScanCover.add"
        need(not self.finished, "%s: the last pass has been added" % what)
        need(last or (counts is None and not want_pred), "%s: counts and predictions come with the last pass (last=True)" % what)
        need(isinstance(batch, dict) and all(k in batch for k in ("sel", "cover", "scans", "sizes", "scan_ids")),
             "%s: batch must come from a ValBatcher's or VoteBatcher's cover() (sel, cover, scans, sizes, scan_ids)" % what)
        p, passes, rnd = (int(v) for v in batch["cover"])
        need(0 <= p < passes and rnd >= 0, "%s: batch cover = (pass, passes, round), got %r" % (what, batch["cover"]))
        need(not last or p + 1 == passes, "%s: the arg-max is taken on the last pass of a round (pass %d of %d)" % (what, p, passes))
        need(batch["scans"] is self.scans and [int(m) for m in batch["sizes"]] == self.sizes,
             "%s: every pass's batch holds the same scans in the same slots" % what)
        dev, b = self.device, len(self.sizes)
        need(torch.is_tensor(logits), "%s: logits must be a torch.Tensor" % what)
        need(logits.is_cuda, "%s: CPU not supported (logits must live on the GPU)" % what)
        need(logits.dim() == 3 and logits.shape[1] == self.c and logits.dtype == torch.float32, "%s: fp32 logits (B, %d, N)" % (what, self.c))
        need(logits.device == dev, "%s: logits on %s, the scans on %s" % (what, logits.device, dev))
        n = int(logits.shape[2])
        need(logits.shape[0] == b and n >= 1, "%s: %d logits rows for a batch of %d scans, N >= 1" % (what, logits.shape[0], b))
        sel, scan_ids = batch["sel"], batch["scan_ids"]
        need(torch.is_tensor(sel) and sel.device == dev and sel.dtype == torch.int64 and tuple(sel.shape) == (b, n),
             "%s: batch sel must be (B, N) int64 on %s" % (what, dev))
        need(torch.is_tensor(scan_ids) and scan_ids.device == dev and scan_ids.dtype == torch.int64 and tuple(scan_ids.shape) == (b,),
             "%s: batch scan_ids must be (B,) int64 on %s" % (what, dev))
        prob = F.softmax(logits, dim=1).contiguous()
        sel, scan_ids = sel.contiguous(), scan_ids.contiguous()
        pred = torch.empty(sum(self.sizes), dtype=torch.int64, device=dev) if want_pred else None
        mode = (_lib.VOTE_SET if rnd == 0 else 0) | (_lib.VOTE_FINISH if last else 0)
        call("geot_scan_cover", dev, b, self.c, n, len(self.scans), int(self.scans.points.shape[0]), ptr(self.scans.labels),
             ptr(self.scans.offsets), ptr(scan_ids), ptr(sel), ptr(prob), p, int(self.work.shape[0]), ptr(self.work),
             ptr(self.out_offsets), ptr(self.acc), mode, ptr(pred), ptr(counts))
        if p + 1 == passes:
            self.rounds = rnd + 1
        self.finished = bool(last)
        return [q.view(1, -1) for q in torch.split(pred, self.sizes)] if want_pred else None

    def probabilities(self):
        """Per scan the (M_i, C) mean over the complete rounds so far: the accumulator's rows times 1 / rounds."""
        need(self.rounds >= 1, "ScanCover.probabilities: no complete round yet")
        return list(torch.split(self.acc * (1.0 / self.rounds), self.sizes))


def _rounds(rounds, what):
    if isinstance(rounds, bool) or not isinstance(rounds, (int, np.integer)) or int(rounds) < 1:
        raise ValueError("%s: rounds must be an int >= 1, got %r" % (what, rounds))
    return int(rounds)


def _cover_run(model, batcher, idx, rounds, interpolate, draws, graph, lookahead, what, num_classes=None, counts=None, want_pred=True):
    """The covering passes of one batch of scans through _passes: rounds * P forward passes on batcher.cover(idx, ...)'s
    batches, summed by a ScanCover (interpolate: a ScanVotes, geot_scan_vote on the same batches) and finished on the last
    -> (the labels or None, the last batch, the class count).  lookahead=True is G = P: one geometry call per round."""
    from .openpoints.dataset.sample_draw import cover_passes
    ids = [int(i) for i in idx]
    feed = batcher.cover(ids, rounds, draws)                # the checks of idx, rounds and draws, before any device call
    passes = cover_passes([batcher.scans.sizes[i] for i in ids], batcher.m)
    lookahead, graphed = _replay_switches(graph, lookahead, passes, model, what)
    sums = preds = data = None
    for data, logits, first, last in _passes(model, batcher, [ids], passes * rounds, None, lookahead, graphed,
                                             feed=lambda k: next(feed)):
        if first:
            sums = (ScanVotes if interpolate else ScanCover)(data, logits.shape[1] if num_classes is None else num_classes)
        preds = sums.add(logits, data, last=last, counts=counts if last else None, want_pred=want_pred and last)
    return preds, data, sums.c


@torch.no_grad()
def cover_scans(model, batcher, idx, rounds=1, interpolate=False, draws=None, refine=0, parts=None, graph=False, lookahead=0,
                islands=None):
    """The per-vertex labels of the scans `idx` of a ValBatcher's or VoteBatcher's set from covering passes: list of (1, M_i)
    int64 tensors, as predict_scans returns them.  P = cover_passes(sizes, m) model passes per round whose samples partition
    every scan (batcher.cover), so each vertex takes the arg-max of the probabilities the model produced for that very vertex,
    summed over `rounds` independent covers -- geot_scan_cover, no neighbour search and no interpolation.  draws: a DeviceDraws
    for these batches (default: the batcher's; ValueError without one).  interpolate=True sends the same batches through
    ScanVotes / geot_scan_vote instead: a vertex gets its own pass's value (weight about 1 at distance about 0) plus P - 1
    interpolated ones.  refine, parts: the labels then go through refine_scans.  graph, lookahead: as for vote_scans;
    lookahead=True runs one geometry call per round.  islands: as for predict_scans."""
    n_refine = _refine_n(refine, "cover_scans")
    islands = _islands_kw(islands, "cover_scans")
    rounds = _rounds(rounds, "cover_scans")
    _need_mesh(islands, batcher, "cover_scans")
    model.eval()
    preds, data, c = _cover_run(model, batcher, idx, rounds, interpolate, draws, graph, lookahead, "cover_scans")
    return _finish_labels(preds, data, n_refine, parts, islands, c)


@torch.no_grad()
def validate_scans_covered(model, scans, cfg, rounds=1, interpolate=False, batch_size=2, indices=None, stream=None, draws=None,
                           refine=0, parts=None, graph=False, lookahead=0, teeth=None, islands=None):
    """validate_scans scored on covering passes: every batch of scans runs through the model rounds * P times (cover_scans),
    each vertex scored on the class the model gave that very vertex.  scans: a DeviceScanSet (a ValBatcher is built on it:
    cfg.num_points, cfg.num_classes), or a ValBatcher / VoteBatcher built on one (a VoteBatcher applies its vote list per
    pass).  draws: a DeviceDraws (default: the batcher's; ValueError without one).  Same log lines, return value and dtypes as
    validate().  interpolate, refine, parts, graph, lookahead: as for cover_scans.  teeth: as for validate_scans (the last pass's
    finish writes the labels beside the counts).  islands: as for validate_scans."""
    from .openpoints.dataset.val_batch import ScanBatcher, ValBatcher
    what = "validate_scans_covered"
    n_refine = _refine_n(refine, what)
    islands = _islands_kw(islands, what)
    rounds = _rounds(rounds, what)
    need(int(batch_size) >= 1, "%s: batch_size >= 1" % what)
    model.eval()
    c = _cfg(cfg, "num_classes", 17)
    if isinstance(scans, ScanBatcher):
        batcher = scans
        need(stream is None or stream is batcher.stream, "%s: the batcher was built for another stream" % what)
    else:
        need(_cfg(cfg, "num_points") is not None, "%s: cfg.num_points (the sample size) is missing" % what)
        batcher = ValBatcher(scans, _cfg(cfg, "num_points"), c, stream=stream, draws=draws)
    _need_mesh(islands, batcher, what)
    order = list(range(len(batcher))) if indices is None else [int(i) for i in indices]
    metrics = SegMetrics(c, batcher.device)
    _need_teeth(teeth, c, batcher.device, what)
    for at in range(0, len(order), int(batch_size)):
        ids = order[at:at + int(batch_size)]
        if n_refine or islands is not None:
            preds, data, _ = _cover_run(model, batcher, ids, rounds, interpolate, draws, graph, lookahead, what, c)
            preds = _count_refined(metrics, preds, data, n_refine, parts, islands)
        else:
            rows = metrics._rows(len(ids))
            preds, data, _ = _cover_run(model, batcher, ids, rounds, interpolate, draws, graph, lookahead, what, c, counts=rows,
                                        want_pred=teeth is not None)
            metrics.mandible += [batcher.cls_host[i] == 0 for i in ids]
        if teeth is not None:
            teeth.update(preds, data)
    return _report(metrics.read(), cfg)


# ---- whole scans decoded at full resolution from one backbone pass (csrc/scan_decode.hip) ------------------------------------------
DECODE_RECORD = 256     # vertices per work record: geot_scan_decode_front takes a record 256 vertices at a time, one lane each


def decode_work_table(sizes, chunk=32768, record=DECODE_RECORD):
    """The work records of geot_scan_decode_front / geot_scan_decode_finish for batch slots of `sizes` vertices, decoded in
    chunks of at most `chunk` vertices -> ((G, 4) int32 host array of (slot, first vertex, vertex count, first output row),
    [(first record, record count, rows)] per chunk).  The vertices of all slots, slot after slot, are cut every `chunk`
    vertices -- a boundary may fall inside a scan -- and every piece into records of at most `record` vertices; a record's
    rows are counted from the start of ITS chunk, so one (chunk, c_out) buffer serves every chunk.  Every vertex of every slot
    lies in exactly one record."""
    sizes = [int(m) for m in sizes]
    need(all(1 <= m <= MAX_VERTICES for m in sizes), "decode_work_table: 1 .. %d vertices per scan" % MAX_VERTICES)
    need(isinstance(chunk, (int, np.integer)) and not isinstance(chunk, bool) and 1 <= int(chunk) <= MAX_VERTICES and int(record) >= 1,
         "decode_work_table: chunk must be an int in 1 .. %d, record >= 1" % MAX_VERTICES)
    chunk, record = int(chunk), int(record)
    rows, chunks, at, n_rec, first_rec = [], [], 0, 0, 0       # at: vertices handed out so far
    for slot, m in enumerate(sizes):
        v = 0
        while v < m:
            used = at % chunk
            take = min(m - v, chunk - used)
            first = np.arange(v, v + take, record, dtype=np.int64)
            part = np.empty((first.size, 4), dtype=np.int64)
            part[:, 0], part[:, 1], part[:, 2], part[:, 3] = slot, first, np.minimum(record, v + take - first), used + first - v
            rows.append(part)
            n_rec += first.size
            at += take
            v += take
            if at % chunk == 0:
                chunks.append((first_rec, n_rec - first_rec, chunk))
                first_rec = n_rec
    if at % chunk:
        chunks.append((first_rec, n_rec - first_rec, at % chunk))
    table = np.concatenate(rows) if rows else np.zeros((0, 4), dtype=np.int64)
    return np.ascontiguousarray(table.astype(np.int32)), chunks


def _decode_run(model, batcher, ids, c, draws, chunk, what, counts=None, want_pred=True, debug=None, sel=None):
    """One batch of scans decoded: one batch() with the view affine, one forward pass that keeps the last stage's inputs, then
    per chunk of vertices geot_scan_decode_front, the model's decode_tail and geot_scan_decode_finish
    -> (the labels as predict_scans returns them or None, the batch).  No host synchronisation.
    debug (tests): a list; per chunk a dict is appended -- work (the chunk's records, host), logits (C, rows), and the kernel's
    optional outputs q / idx / weight (rows, 3); first comes a dict of the batch's own logits "forward" (B, C, N), the folded
    "params" and the kept "state".  sel: the
    batch's vertex samples, given."""
    seg = getattr(model, "segmentor", model)
    need(hasattr(seg, "decode_front_params") and hasattr(seg, "decode_tail"),
         "%s: the model has no last stage to decode with (PointTransformer_seg_T.decode_front_params / decode_tail)" % what)
    if seg.training:
        raise ValueError("%s: eval mode only (model.eval()): a training-mode BatchNorm ties every point to its batch" % what)
    data = batcher.batch(ids, sel=sel, draws=draws, affine=True)
    batcher.join(data)
    if "pos_search" in data:            # a VoteBatcher: the affine describes the `val` view, so that is the view decoded
        data = dict(data, pos=data["pos_search"])
    keep, seg.keep_decode_state = seg.keep_decode_state, True
    try:
        forward = model(data)[0]
        p, state = seg.decode_front_params(), seg.decode_state
    finally:
        seg.keep_decode_state, seg.decode_state = keep, None
    scans, sizes = data["scans"], [int(m) for m in data["sizes"]]
    dev, b = scans.device, len(sizes)
    need(1 <= b <= SCAN_MAX_SLOTS, "%s: 1 .. %d scans per batch" % (what, SCAN_MAX_SLOTS))
    m, c_out = int(p["a"].shape[1]), int(p["a"].shape[2])
    need(tuple(p["known"].shape) == (b, m, 3) and m >= 3, "%s: the model kept %s centres for %d scans (at least 3 each)" %
         (what, tuple(p["known"].shape), b))
    table, chunks = decode_work_table(sizes, chunk)
    work = _to_device(table, dev)
    scan_ids = data["scan_ids"].contiguous()
    center, scale = data["center"].contiguous(), data["scale"].contiguous()
    vcenter, vscale = data["view_center"].contiguous(), data["view_scale"].contiguous()
    out_offs = _out_offsets(sizes, dev) if want_pred else None
    pred = torch.empty(sum(sizes), dtype=torch.int64, device=dev) if want_pred else None
    z = torch.empty((max(r for _, _, r in chunks), c_out), dtype=torch.float32, device=dev)
    n_scans, total = len(scans), int(scans.points.shape[0])
    if debug is not None:
        debug.append({"forward": forward, "params": p, "state": state})
    for first, count, rows in chunks:
        recs = ptr(work) + 16 * first
        seen = None
        if debug is not None:
            seen = {"q": torch.empty((rows, 3), dtype=torch.float32, device=dev), "idx": torch.empty((rows, 3), dtype=torch.int32, device=dev),
                    "weight": torch.empty((rows, 3), dtype=torch.float32, device=dev)}
        call("geot_scan_decode_front", dev, b, m, c_out, int(p["relu"]), n_scans, total, ptr(scans.points), ptr(scans.offsets),
             ptr(scan_ids), ptr(center), ptr(scale), ptr(vcenter), ptr(vscale), ptr(p["known"]), ptr(p["a"]), ptr(p["skip_const"]),
             ptr(p["w_xyz"]), ptr(p["ch_scale"]), ptr(p["ch_shift"]), count, recs, rows, ptr(z),
             *((ptr(seen["q"]), ptr(seen["idx"]), ptr(seen["weight"])) if seen else (None, None, None)))
        logits = seg.decode_tail(z[:rows]).contiguous()
        if seen is not None:
            debug.append(dict(seen, work=table[first:first + count], logits=logits))
        need(tuple(logits.shape) == (c, rows) and logits.dtype == torch.float32, "%s: the head gave %s logits for %d classes and %d "
             "vertices" % (what, tuple(logits.shape), c, rows))
        call("geot_scan_decode_finish", dev, b, c, n_scans, total, ptr(scans.labels), ptr(scans.offsets), ptr(scan_ids), count, recs,
             rows, ptr(logits), ptr(out_offs), ptr(pred), ptr(counts))
    return ([q.view(1, -1) for q in torch.split(pred, sizes)] if want_pred else None), data


@torch.no_grad()
def decode_scans(model, batcher, idx, refine=0, parts=None, chunk=32768, draws=None, islands=None):
    """The per-vertex labels of the scans `idx` of a ValBatcher's or VoteBatcher's set, every vertex predicted directly from
    ONE forward pass: list of (1, M_i) int64 tensors, as predict_scans returns them.  The model sees one sampled batch; its
    last decoder stage (propogation_0, seg_head) is then evaluated at EVERY vertex of the scans -- geot_scan_decode_front takes
    a vertex through the batch's two normalisations, finds its three nearest of the model's 8192 centres and writes the
    stage's first activations, the model's own code does the rest (decode_tail), geot_scan_decode_finish takes the arg-max --
    `chunk` vertices at a time (what bounds the (chunk, 1536) fp32 buffer: 201 MB at the default).  Eval mode only (ValueError
    for a model in training mode).  A VoteBatcher's batch is decoded on its `val` view; votes and rounds do not apply.  refine
    (0: off, True: n = 10, an int: n) and parts: the labels then go through refine_scans.  draws: a DeviceDraws for the
    batch (default: the batcher's).  What this computes is the model's own decoder at those positions; how decoded labels
    compare with interpolated or covered ones on real scans has not been measured (there are no trained weights here).
    islands: as for predict_scans."""
    n_refine = _refine_n(refine, "decode_scans")
    islands = _islands_kw(islands, "decode_scans")
    _need_mesh(islands, batcher, "decode_scans")
    seg = getattr(model, "segmentor", model)
    c = _need_classes(getattr(seg, "nclasses", batcher.c), "decode_scans")
    preds, data = _decode_run(model, batcher, [int(i) for i in idx], c, draws, chunk, "decode_scans")
    return _finish_labels(preds, data, n_refine, parts, islands, c)


@torch.no_grad()
def validate_scans_decoded(model, scans, cfg, batch_size=2, indices=None, stream=None, draws=None, refine=0, parts=None, chunk=32768,
                           teeth=None, islands=None):
    """validate_scans scored on decoded labels (decode_scans): per batch of scans one batch() and one forward pass, then the
    last decoder stage at every vertex, counted by geot_scan_decode_finish.  scans: a DeviceScanSet (a ValBatcher is built on
    it: cfg.num_points, cfg.num_classes), or a ValBatcher / VoteBatcher built on one.  Same log lines, return value and
    dtypes as validate().  refine, parts: as for validate_scans; chunk, draws: as for decode_scans.  No host synchronisation
    beyond validate_scans' (the final read of the counts).  teeth: as for validate_scans (every chunk's finish writes its
    labels beside the counts).  islands: as for validate_scans."""
    from .openpoints.dataset.val_batch import ScanBatcher, ValBatcher
    what = "validate_scans_decoded"
    n_refine = _refine_n(refine, what)
    islands = _islands_kw(islands, what)
    need(int(batch_size) >= 1, "%s: batch_size >= 1" % what)
    model.eval()                        # as validate_scans; decode_scans itself refuses a model in training mode
    c = _need_classes(_cfg(cfg, "num_classes", 17), what)
    if isinstance(scans, ScanBatcher):
        batcher = scans
        need(stream is None or stream is batcher.stream, "%s: the batcher was built for another stream" % what)
    else:
        need(_cfg(cfg, "num_points") is not None, "%s: cfg.num_points (the sample size) is missing" % what)
        batcher = ValBatcher(scans, _cfg(cfg, "num_points"), c, stream=stream, draws=draws)
    _need_mesh(islands, batcher, what)
    order = list(range(len(batcher))) if indices is None else [int(i) for i in indices]
    metrics = SegMetrics(c, batcher.device)
    _need_teeth(teeth, c, batcher.device, what)
    for at in range(0, len(order), int(batch_size)):
        ids = order[at:at + int(batch_size)]
        if n_refine or islands is not None:
            preds, data = _decode_run(model, batcher, ids, c, draws, chunk, what)
            preds = _count_refined(metrics, preds, data, n_refine, parts, islands)
        else:
            rows = metrics._rows(len(ids))
            preds, data = _decode_run(model, batcher, ids, c, draws, chunk, what, counts=rows, want_pred=teeth is not None)
            metrics.mandible += [batcher.cls_host[i] == 0 for i in ids]
        if teeth is not None:
            teeth.update(preds, data)
    return _report(metrics.read(), cfg)


# ---- the Teeth3DS challenge scores: TSA, TLA, TIR (csrc/tooth_scores.hip) -----------------------------------------------------------
TOOTH_ENTRIES = 21          # int64 per class in a geot_tooth_moments row (include/geot_hip.h); the row ends with two slot entries
TOOTH_BIAS = 1 << 30        # the extents are stored as max(q + 2^30) and max(2^30 - q)
TOOTH_SCALE = 65536.0       # q = rint((p - center) * 65536)
TLA_PENALTY = 5.0           # a true tooth's normalised distance when the scan has no predicted tooth (the challenge's penalty)
TIR_RADIUS = 0.5            # a true tooth is identified when its nearest predicted centroid lies closer than half its size
# The moments kernel is set by launch cost and atomics, not by memory (profiles/tooth_scores_timing.txt), and one vertex costs a
# lane far less than geot_scan_predict's search: its records are cut longer, one vertex per lane of a 256-thread workgroup.
TOOTH_CHUNK_MIN = 256


def _mean(values):
    values = [v for v in values if not np.isnan(v)]
    return float(np.mean(values)) if values else float("nan")


def tooth_scores_from_moments(moments, centers, num_classes, mandible):
    """ToothScores.read()'s host half (no device needed; numpy float64): moments (S, 21 C + 2) int64 as geot_tooth_moments
    writes them, centers (S, 3) the origin each scan was quantised around, mandible (S,) the jaw flags -> a dict.

    These definitions restate the published 3DTeethSeg'22 evaluation; the challenge's own script was not available to test
    against, so agreement with it is not tested.  Teeth are the classes 1 .. C - 1.  Per scan and class, from the moments:
    centroid = center + (sum / count) / 65536; size of a TRUE tooth = its per-axis extent (max - min) / 65536, a 3-vector;
    G = the true teeth present, P = the predicted teeth present.  A true tooth with a zero extent on any axis is `degenerate`:
    reported, and left out of TLA and TIR (numerators and denominators).  Per scan:
      tla           for every true tooth t the predicted tooth u* whose centroid is nearest in plain Euclidean distance (the
                    lowest class among equals), d_t = ||(g_t - p_u*) / size_t||_2 divided per axis; with P empty d_t = 5;
                    the mean of d_t over G (NaN for a scan whose true teeth are all degenerate);
      tir           the share of G with d_t < 0.5 and u* == t;
      tsa           the agreement of (label != 0) with (pred != 0) over the usable vertices with a label in [0, C):
                    (tooth on both sides + gingiva on both sides) / vertices -- the micro-averaged F1 of the tooth / gingiva
                    split, as the challenge's script scores a jaw;
      tsa_instance  the mean over G (degenerate teeth included) of 2 hit_t / (n_label_t + n_pred_t), the per-tooth F1 of the
                    challenge paper's text.
    Over the epoch: "tla", "tsa", "tsa_instance" are means over the scans that have a true tooth (tla: one that is not
    degenerate); "tir" is pooled, hits over all true teeth; "exp_neg_tla" = exp(-tla); "score" = (tsa + exp_neg_tla + tir) / 3.
    Also returned: the per-scan lists "tsa_list", "tsa_instance_list", "tla_list", "tir_list", "teeth_list" (|G| without the
    degenerate) and "hits_list"; per jaw "mandible_tsa" ... "maxillary_tir" (tir pooled per jaw); "degenerate" [(scan, class)];
    "unusable" (positions that were not finite or lay 16384 units or more from their centre; a warning is logged when it is not
    zero) and "scans"."""
    c = int(num_classes)
    words = TOOTH_ENTRIES * c + 2
    rows = np.asarray(moments, dtype=np.int64).reshape(-1, words)
    centers = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
    need(len(mandible) == rows.shape[0] == centers.shape[0], "ToothScores: %d jaw flags and %d centres for %d scans" %
         (len(mandible), centers.shape[0], rows.shape[0]))
    tsa_l, tsai_l, tla_l, tir_l, teeth_l, hits_l, degenerate = [], [], [], [], [], [], []
    for i, row in enumerate(rows):
        m = row[:TOOTH_ENTRIES * c].reshape(c, TOOTH_ENTRIES)
        both, n_label, n_pred, hit = int(row[-2]), m[:, 0], m[:, 10], m[:, 20]
        G = [k for k in range(1, c) if n_label[k] > 0]
        P = [k for k in range(1, c) if n_pred[k] > 0]
        if not G:
            for lst in (tsa_l, tsai_l, tla_l, tir_l):
                lst.append(float("nan"))
            teeth_l.append(0)
            hits_l.append(0)
            continue
        tsa_l.append((both + int(hit[0])) / int(n_label.sum()))
        tsai_l.append(float(np.mean([2.0 * hit[k] / (n_label[k] + n_pred[k]) for k in G])))
        p_cent = np.array([centers[i] + (m[k, 11:14] / float(n_pred[k])) / TOOTH_SCALE for k in P]).reshape(-1, 3)
        dist, hits, used = [], 0, 0
        for t in G:
            size = (m[t, 4:7] + m[t, 7:10] - 2 * TOOTH_BIAS) / TOOTH_SCALE
            if (size == 0).any():
                degenerate.append((i, t))
                continue
            used += 1
            if not P:
                dist.append(TLA_PENALTY)
                continue
            g = centers[i] + (m[t, 1:4] / float(n_label[t])) / TOOTH_SCALE
            u = int(np.argmin(np.sqrt(((p_cent - g) ** 2).sum(1))))         # the first minimum: the lowest class among equals
            d = float(np.sqrt((((g - p_cent[u]) / size) ** 2).sum()))
            dist.append(d)
            hits += int(d < TIR_RADIUS and P[u] == t)
        tla_l.append(float(np.mean(dist)) if used else float("nan"))
        tir_l.append(hits / used if used else float("nan"))
        teeth_l.append(used)
        hits_l.append(hits)
    unusable = int(rows[:, -1].sum()) if len(rows) else 0
    if unusable:
        logging.warning("ToothScores: %d vertex positions were not finite or lay 16384 units or more from their centre; they "
                        "are in no score" % unusable)

    def over(sel):
        teeth = sum(teeth_l[i] for i in sel)
        return dict(tsa=_mean([tsa_l[i] for i in sel]), tsa_instance=_mean([tsai_l[i] for i in sel]),
                    tla=_mean([tla_l[i] for i in sel]), tir=sum(hits_l[i] for i in sel) / teeth if teeth else float("nan"))
    out = over(range(len(rows)))
    out["exp_neg_tla"] = float(np.exp(-out["tla"]))
    out["score"] = (out["tsa"] + out["exp_neg_tla"] + out["tir"]) / 3.0
    for jaw, lower in (("mandible", True), ("maxillary", False)):
        for key, v in over([i for i, flag in enumerate(mandible) if bool(flag) == lower]).items():
            out["%s_%s" % (jaw, key)] = v
    out.update(tsa_list=tsa_l, tsa_instance_list=tsai_l, tla_list=tla_l, tir_list=tir_l, teeth_list=teeth_l, hits_list=hits_l,
               degenerate=degenerate, unusable=unusable, scans=len(rows))
    return out


def _tooth_launch(preds, batch, c, rows, what):
    """One geot_tooth_moments call: the per-scan labels `preds` of a ValBatcher / VoteBatcher batch against the scans' own
    labels and positions, read in place from the set, ADDED into `rows` (b, 21 c + 2) int64.  No host synchronisation."""
    need(isinstance(batch, dict) and all(k in batch for k in ("center", "scan_ids", "scans", "sizes")),
         "%s: batch must come from ValBatcher.batch / VoteBatcher.batch (center, scan_ids, scans, sizes)" % what)
    scans, sizes = batch["scans"], [int(m) for m in batch["sizes"]]
    dev, b = scans.device, len(sizes)
    need(isinstance(preds, (list, tuple)) and len(preds) == b and 1 <= b <= SCAN_MAX_SLOTS,
         "%s: one prediction tensor per scan of the batch (1 .. %d)" % (what, SCAN_MAX_SLOTS))
    for p, m in zip(preds, sizes):
        need(torch.is_tensor(p) and p.dtype == torch.int64, "%s: the predictions must be int64 tensors" % what)
        need(p.numel() == m, "%s: %d predictions for a scan of %d vertices" % (what, p.numel(), m))
        need(p.is_cuda and p.device == dev, "%s: CPU not supported (the predictions must live on %s, with the scans)" % (what, dev))
    for key, dt, shape in (("center", torch.float32, (b, 3)), ("scan_ids", torch.int64, (b,))):
        need(torch.is_tensor(batch[key]) and batch[key].device == dev and batch[key].dtype == dt and tuple(batch[key].shape) == shape,
             "%s: batch %s must be a %s %s tensor on %s" % (what, key, shape, dt, dev))
    flat, _ = _flat_labels(preds, sizes, dev)
    center, scan_ids = batch["center"].contiguous(), batch["scan_ids"].contiguous()
    work = _to_device(scan_work_table(sizes, min_chunk=TOOTH_CHUNK_MIN), dev)
    call("geot_tooth_moments", dev, b, c, len(scans), int(scans.points.shape[0]), ptr(scans.points), ptr(scans.labels),
         ptr(scans.offsets), ptr(scan_ids), ptr(center), int(work.shape[0]), ptr(work), ptr(_out_offsets(sizes, dev)), ptr(flat),
         ptr(rows))
    return center


class ToothScores:
    """The Teeth3DS challenge scores of one epoch -- TSA, TLA, TIR (tooth_scores_from_moments) -- from moments taken on the
    device: a (scans, 21 C + 2) int64 buffer and the (scans, 3) fp32 centres the scans were quantised around (capacities double
    as scans arrive; both stay on the device until read()), and each scan's jaw, kept on the host.  update() does not
    synchronise with the host."""

    def __init__(self, num_classes, device):
        c = _need_classes(num_classes, "ToothScores")
        dev = torch.device(device)
        need(dev.type == "cuda", "ToothScores: the moments live on a GPU, got device %s" % dev)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.c, self.words, self.device = c, TOOTH_ENTRIES * c + 2, dev
        self.moments = torch.zeros((8, self.words), dtype=torch.int64, device=dev)
        self.centers = torch.zeros((8, 3), dtype=torch.float32, device=dev)
        self.mandible = []

    @property
    def scans(self):
        return len(self.mandible)

    def reset(self):
        """A new epoch."""
        self.moments.zero_()
        self.mandible = []

    def _rows(self, b):
        """The (zero) moment rows and the centre rows of the next b scans."""
        n0 = self.scans
        if n0 + b > self.moments.shape[0]:
            cap = max(n0 + b, 2 * self.moments.shape[0])
            for name in ("moments", "centers"):
                old = getattr(self, name)
                grown = torch.zeros((cap, old.shape[1]), dtype=old.dtype, device=self.device)
                grown[:n0].copy_(old[:n0])
                setattr(self, name, grown)
        return self.moments[n0:n0 + b], self.centers[n0:n0 + b]

    def update(self, preds, batch):
        """One batch: preds as predict_scans / vote_scans / cover_scans / decode_scans return them -- per scan of the batch a
        (1, M_i) int64 tensor -- and the ValBatcher / VoteBatcher batch they belong to (its scans, scan_ids, sizes, center and
        jaw flags).  One geot_tooth_moments call, no host synchronisation."""
        need(isinstance(batch, dict) and "mandible" in batch and "scans" in batch and "sizes" in batch,
             "ToothScores.update: batch must come from ValBatcher.batch / VoteBatcher.batch")
        need(batch["scans"].device == self.device, "ToothScores.update: the scans on %s, the moments on %s" %
             (batch["scans"].device, self.device))
        flags = [bool(m) for m in batch["mandible"]]
        need(len(flags) == len(batch["sizes"]), "ToothScores.update: one jaw flag per scan")
        rows, centers = self._rows(len(flags))
        centers.copy_(_tooth_launch(preds, batch, self.c, rows, "ToothScores.update"))
        self.mandible += flags

    def read(self):
        """The epoch so far, in one device-to-host copy (the moments and the centres travel as one buffer) -> the dict of
        tooth_scores_from_moments."""
        n = self.scans
        packed = torch.cat([self.moments[:n].view(torch.uint8).reshape(n, -1), self.centers[:n].view(torch.uint8).reshape(n, -1)], 1).cpu().numpy()
        moments = np.ascontiguousarray(packed[:, :8 * self.words]).view(np.int64)
        centers = np.ascontiguousarray(packed[:, 8 * self.words:]).view(np.float32)
        return tooth_scores_from_moments(moments, centers, self.c, self.mandible)


def _need_teeth(teeth, c, dev, what):
    """The validators' teeth= keyword: None or a ToothScores of the same class count on the scans' device."""
    if teeth is None:
        return
    need(isinstance(teeth, ToothScores), "%s: teeth must be a ToothScores or None, got %r" % (what, type(teeth).__name__))
    dev = torch.device(dev)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    need(teeth.c == int(c) and teeth.device == dev, "%s: teeth counts %d classes on %s, the validation %d on %s" %
         (what, teeth.c, teeth.device, int(c), dev))


@torch.no_grad()
def tooth_instances(preds, batch, num_classes):
    """The geometry of the predicted teeth, for users who want more than the scores: preds and batch as ToothScores.update takes
    them -> a dict of device tensors, per scan of the batch and class: "count" (B, C) int64 predicted vertices; "centroid"
    (B, C, 3) fp64; "box_min" / "box_max" (B, C, 3) fp64, the axis-aligned box -- in the scans' coordinates, to the 2^-16 of a
    unit the moments resolve, NaN for a class that was not predicted.  The same single geot_tooth_moments launch, then a few
    torch statements on the (B, 21 C + 2) row buffer; no host synchronisation."""
    c = _need_classes(num_classes, "tooth_instances")
    need(isinstance(batch, dict) and "scans" in batch and "sizes" in batch, "tooth_instances: batch must come from ValBatcher.batch")
    dev, b = batch["scans"].device, len(batch["sizes"])
    rows = torch.zeros((b, TOOTH_ENTRIES * c + 2), dtype=torch.int64, device=dev)
    center = _tooth_launch(preds, batch, c, rows, "tooth_instances").double().view(b, 1, 3)
    m = rows[:, :TOOTH_ENTRIES * c].view(b, c, TOOTH_ENTRIES)
    count = m[:, :, 10]
    empty = (count == 0).view(b, c, 1)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    centroid = center + (m[:, :, 11:14].double() / count.double().view(b, c, 1)) / TOOTH_SCALE
    box_max = center + (m[:, :, 14:17] - TOOTH_BIAS).double() / TOOTH_SCALE
    box_min = center + (TOOTH_BIAS - m[:, :, 17:20]).double() / TOOTH_SCALE
    return {"count": count.clone(), "centroid": torch.where(empty, nan, centroid), "box_min": torch.where(empty, nan, box_min),
            "box_max": torch.where(empty, nan, box_max)}


def report_tooth_scores(out, cfg):
    """The one log line of the challenge scores, in the style of validate's three."""
    epoch = "%s/%s" % (_cfg(cfg, "epoch"), _cfg(cfg, "epochs"))
    logging.info(f"Test Epoch [{epoch}],TSA {out['tsa']:.5f}, TSA(instance) {out['tsa_instance']:.5f}, TLA {out['tla']:.5f}, "
                 f"TIR {out['tir']:.5f}, score {out['score']:.5f}")
