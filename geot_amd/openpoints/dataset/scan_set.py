"""Scans that live on the GPU and the batch sampling on them: what every batcher of this package (batcher.py and the three
modules built on it) starts from.  DeviceScanSet holds the scans of one split; cloud_sample_batch (geot_cloud_sample_batch,
csrc/dataprep.hip) draws nothing itself: it gathers the given vertex indices of every batch slot and normalises them as the
reference's dataset does per item (openpoints/dataset/tooth_semi/tooth_dataset.py:116-147)."""
import numpy as np
import torch

from ... import _lib
from ...ext._common import call, need, ptr


def _to_device(host, dev):
    """Pinned staging + non-blocking copy on the current stream: no synchronisation (validation.SegMetrics._offsets)."""
    return torch.from_numpy(host).pin_memory().to(dev, non_blocking=True)


def check_faces(faces, n):
    """DeviceScanSet's host checks of `faces`, before any upload and before the device is looked at: one entry per scan, each
    None (a scan without a mesh) or an (F_i >= 0, 3) integer array or tensor -> the entries as host tensors (None kept).  The
    index VALUES are not checked: geot_mesh_neighbours ignores a face with an index outside its scan and counts it."""
    need(isinstance(faces, (list, tuple)) and len(faces) == n,
         "DeviceScanSet: faces must be a sequence with one entry per scan (%d): an (F, 3) integer array, or None" % n)
    out = []
    for i, f in enumerate(faces):
        if f is None:
            out.append(None)
            continue
        t = torch.as_tensor(f)
        need(t.dim() == 2 and t.shape[1] == 3, "DeviceScanSet: faces[%d] must be (F, 3), got %s" % (i, tuple(t.shape)))
        need(not t.is_floating_point() and not t.is_complex() and t.dtype != torch.bool,
             "DeviceScanSet: faces[%d] must hold integer vertex indices, got %s" % (i, t.dtype))
        out.append(t)
    return out


class DeviceScanSet:
    """The scans of one split on one device, built once: vertices concatenated (sum N, 3) float32, labels (sum N,) int32,
    offsets (n + 1,) int64, the jaw flag of every scan `cls` (n,) int64 (tooth_dataset.py:97, 0 = lower; default 0).
    scans / labels: sequences of (N_i, 3) / (N_i,) arrays or tensors.
    faces (default None: the set holds no meshes and `faces`, `face_offsets`, `face_sizes` and `has_mesh` are None): a sequence
    with one entry per scan, an (F_i, 3) integer array or tensor of vertex indices local to the scan (io.read_obj's second
    result), or None for a scan without a mesh.  Stored concatenated: faces (sum F, 3) int32 and face_offsets (n + 1,) int64 on
    the device, face_sizes and has_mesh host lists (None: face_sizes[i] = 0 and has_mesh[i] False; an empty (0, 3) array: a mesh
    with no faces).  An index that does not fit int32 is stored as -1 or 2^31 - 1: outside every scan either way.
    keep_tables(): validation.scan_neighbours and mesh_neighbours keep every scan's neighbour table on the set (off by
    default).
    compute_curvature(): the per-vertex discrete Gaussian curvature of the scans with a mesh (`curvature`, `curvature_range`,
    `curvature_radius`, `defects`: None until it is called), what the batchers' curvatures=True gathers from."""

    def __init__(self, scans, labels, cls=None, device=None, faces=None):
        need(len(scans) >= 1 and len(scans) == len(labels), "DeviceScanSet: one label array per scan, at least one scan")
        meshes = None if faces is None else check_faces(faces, len(scans))
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        need(dev.type == "cuda", "DeviceScanSet: CPU not supported (the scans must live on the GPU)")
        pts = [torch.as_tensor(p) for p in scans]
        labs = [torch.as_tensor(l) for l in labels]
        for p, l in zip(pts, labs):
            need(p.dim() == 2 and p.shape[1] == 3 and p.shape[0] >= 1, "DeviceScanSet: a scan is (N>=1, 3)")
            need(l.dim() == 1 and l.shape[0] == p.shape[0] and not l.is_floating_point(),
                 "DeviceScanSet: one integer label per vertex")
        self.sizes = [int(p.shape[0]) for p in pts]
        cls = [0] * len(pts) if cls is None else [int(c) for c in cls]
        need(len(cls) == len(pts), "DeviceScanSet: one cls entry per scan")
        self.device = dev
        self.points = torch.cat([p.to(dev, torch.float32) for p in pts]).contiguous()
        self.labels = torch.cat([l.to(dev, torch.int32) for l in labs]).contiguous()
        self.offsets = torch.tensor(np.concatenate([[0], np.cumsum(self.sizes, dtype=np.int64)]), dtype=torch.int64).to(dev)
        self.cls = torch.tensor(cls, dtype=torch.int64).to(dev)
        self.faces = self.face_offsets = self.face_sizes = self.has_mesh = None
        if meshes is not None:
            self.has_mesh = [f is not None for f in meshes]
            self.face_sizes = [0 if f is None else int(f.shape[0]) for f in meshes]
            host = [f.to(torch.int64).clamp(-1, 2 ** 31 - 1).to(torch.int32) for f in meshes if f is not None]
            self.faces = (torch.cat(host) if host else torch.empty((0, 3), dtype=torch.int32)).to(dev).contiguous()
            self.face_offsets = torch.tensor(np.concatenate([[0], np.cumsum(self.face_sizes, dtype=np.int64)]),
                                             dtype=torch.int64).to(dev)
        self._keep, self._tables = False, {}
        self.curvature = self.curvature_range = self.curvature_radius = self.defects = self._curvature_keys = None
        self._curvature_tables = None

    def __len__(self):
        return len(self.sizes)

    def keep_tables(self, on=True):
        """Switch the per-scan cache of neighbour tables on (or off; off drops what is kept).  While it is on,
        validation.scan_neighbours and validation.mesh_neighbours keep each scan's (M_i, width) int32 table under (scan, "knn" |
        "mesh", width), build only the missing ones and assemble a batch's table from the kept ones with device copies: the
        bits of the uncached call.  Memory: 4 * width * M_i bytes per scan, kind and width (a scan of 1e5 vertices: 3.6 MB for
        the nine-wide kNN table, 6.4 MB for the 16-wide mesh table), held until drop_tables().  The tables depend on the
        vertices and faces alone: whoever changes `points` or `faces` in place calls drop_tables().  Only a batch that carries
        the host scan ids ("ids", which the whole-scan batchers add to every batch they build while the switch is on, and
        always for a set with faces) is served from the cache.  -> self."""
        self._keep = bool(on)
        if not self._keep:
            self._tables = {}
        return self

    def drop_tables(self):
        """Empty the cache of neighbour tables (the switch stays as it is).  The curvature arrays are no cache: they depend on
        the vertices, the faces and the radius, and whoever changes `points` or `faces` in place calls compute_curvature()
        again."""
        self._tables = {}

    def compute_curvature(self, radius=0.1, stats=False):
        """The discrete Gaussian curvature measure of every vertex of every scan with a mesh, on the device: what the
        reference reads from files made offline with trimesh.curvature.discrete_gaussian_curvature_measure(mesh, mesh.vertices,
        radius) (openpoints/dataset/io.py:51-57).  The definition and the rules for unusable faces are include/geot_hip.h's
        (ABI 37), restated from trimesh's documentation; agreement with trimesh itself is not tested.
            defect(v)    = 2 pi - the sum of the face angles at v (boundary vertices too; a vertex in no face: 2 pi)
            curvature(v) = the sum of defect(u) over the scan's vertices u with |u - v| <= radius, v included
        radius is in the scan's RAW units (the reference computes it before pc_norm).  One geot_mesh_angle_defects call over
        all scans with a mesh (three launches) and one geot_scan_ball_sum call per such scan (seven launches), on the current
        stream, without a host synchronisation.  Stores
            curvature        (sum N,) float32, 0 in scans without a mesh
            curvature_range  (n, 2) float32: min and max of |curvature| over each WHOLE scan (0, 0 without a mesh): what the
                             batchers' "curvatures" are normalised with, (|cur| - min) / (max - min), 0 where max == min (the
                             reference's commented code would give NaN there)
            curvature_radius the radius, a float
            defects          (sum N,) int64: the defects as integers, llrint(2 pi 2^32) - sum of llrint(angle 2^32)
        and returns self -- with stats=True the (scans with a mesh, 4) int32 device tensor of usable, ignored (an index outside
        the scan or a repeated one) and degenerate faces (a zero-length edge, a non-finite coordinate) and of vertices in no
        usable face, in scan order.  Calling it again with another radius recomputes.  ValueError, before any device call, for
        a set without faces and for a radius that is not a finite positive number.  The arrays are a pure function of the
        vertices, the faces and the radius: whoever changes `points` or `faces` in place calls it again."""
        r = check_radius(radius, "compute_curvature")
        if self.faces is None:
            raise ValueError("compute_curvature: the scan set holds no faces -- build it with DeviceScanSet(..., faces=)")
        max_scan = _lib.CURVATURE_MAX_SCAN
        meshed = [i for i, has in enumerate(self.has_mesh) if has]
        for i in meshed:
            if self.sizes[i] > max_scan:
                raise ValueError("compute_curvature: scan %d has %d vertices, more than %d" % (i, self.sizes[i], max_scan))
        dev, lib, total, n = self.device, _lib.load(), int(self.points.shape[0]), len(self)
        if self._curvature_tables is None:         # once per set: the slots of the defect calls, 65535 scans at most each
            starts = np.concatenate([[0], np.cumsum(self.sizes, dtype=np.int64)])
            chunks = []
            for first in range(0, len(meshed), 65535):
                part = meshed[first:first + 65535]
                counts = [self.face_sizes[i] for i in part]
                chunks.append((len(part), sum(counts), _to_device(np.asarray(part, dtype=np.int64), dev),
                               _to_device(starts[part].astype(np.int64), dev),
                               _to_device(np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int64), dev)))
            self._curvature_tables = (chunks, starts)
        chunks, starts = self._curvature_tables
        defects = torch.empty(total, dtype=torch.int64, device=dev)
        cur = torch.empty(total, dtype=torch.float32, device=dev)
        if len(meshed) < n:
            defects.fill_(0)
            cur.fill_(0)
        keys = torch.empty((n, 2), dtype=torch.int32, device=dev)
        keys.fill_(-2 ** 31)                        # the key of 0.0 (min = max = 0): what a scan without a mesh keeps
        st = torch.empty((len(meshed), 4), dtype=torch.int32, device=dev) if stats else None
        nbytes = int(lib.geot_mesh_angle_defects_ws_bytes(total))
        need(nbytes >= 0, "geot_mesh_angle_defects: no workspace for %d vertices" % total)
        ws, row = torch.empty(nbytes, dtype=torch.uint8, device=dev), 0
        for b, batch_faces, ids_dev, out_dev, face_out_dev in chunks:
            call("geot_mesh_angle_defects", dev, b, n, total, int(self.faces.shape[0]), ptr(self.points), ptr(self.faces),
                 ptr(self.offsets), ptr(self.face_offsets), ptr(ids_dev), ptr(out_dev), ptr(face_out_dev), batch_faces, total,
                 ptr(defects), ptr(st[row:row + b]) if stats else None, ptr(ws), nbytes)
            row += b
        if meshed:
            nbytes = int(lib.geot_scan_ball_sum_ws_bytes(max(self.sizes[i] for i in meshed)))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            for i in meshed:
                lo, m = int(starts[i]), self.sizes[i]
                call("geot_scan_ball_sum", dev, m, r, ptr(self.points[lo:lo + m]), ptr(defects[lo:lo + m]), ptr(cur[lo:lo + m]),
                     ptr(keys[i]), ptr(ws), nbytes)
        self.curvature, self.defects, self.curvature_radius, self._curvature_keys = cur, defects, r, keys
        self.curvature_range = (keys & 0x7fffffff).view(torch.float32)          # a non-negative float's key: its bits, top bit set
        return st if stats else self

    @classmethod
    def _merged(cls, a, b):
        """a's scans followed by b's, as one set (the batcher samples both splits in one sequence of launches)."""
        need(a.device == b.device, "DeviceScanSet: both sets must be on one device (%s vs %s)" % (a.device, b.device))
        out = cls.__new__(cls)
        out.device, out.sizes = a.device, a.sizes + b.sizes
        out.points, out.labels = torch.cat([a.points, b.points]), torch.cat([a.labels, b.labels])
        out.offsets = torch.cat([a.offsets, b.offsets[1:] + a.offsets[-1:]])
        out.cls = torch.cat([a.cls, b.cls])
        out.faces = out.face_offsets = out.face_sizes = out.has_mesh = None
        if a.faces is not None or b.faces is not None:          # the side without faces: mesh-less scans
            parts = [(s.faces, s.face_sizes, s.has_mesh) if s.faces is not None else
                     (torch.empty((0, 3), dtype=torch.int32, device=s.device), [0] * len(s), [False] * len(s)) for s in (a, b)]
            out.faces = torch.cat([parts[0][0], parts[1][0]])
            out.face_sizes, out.has_mesh = parts[0][1] + parts[1][1], parts[0][2] + parts[1][2]
            out.face_offsets = torch.tensor(np.concatenate([[0], np.cumsum(out.face_sizes, dtype=np.int64)]),
                                            dtype=torch.int64).to(a.device)
        out._keep, out._tables = False, {}
        out.curvature = out.curvature_range = out.curvature_radius = out.defects = out._curvature_keys = None
        out._curvature_tables = None
        if (getattr(a, "curvature", None) is not None and getattr(b, "curvature", None) is not None
                and a.curvature_radius == b.curvature_radius):      # both sides, the same radius: carried over; otherwise dropped
            out.curvature, out.defects = torch.cat([a.curvature, b.curvature]), torch.cat([a.defects, b.defects])
            out._curvature_keys = torch.cat([a._curvature_keys, b._curvature_keys])
            out.curvature_range = torch.cat([a.curvature_range, b.curvature_range])
            out.curvature_radius = a.curvature_radius
        return out


def check_radius(radius, who):
    """A finite positive number that stays one as a float32 -> float; ValueError otherwise (before any device call)."""
    ok = isinstance(radius, (int, float, np.integer, np.floating)) and not isinstance(radius, (bool, np.bool_))
    if ok:
        with np.errstate(over="ignore"):
            as32 = float(np.float32(radius))
        ok = np.isfinite(as32) and as32 > 0.0
    if not ok:
        raise ValueError("%s: radius must be a finite positive number, got %r" % (who, radius))
    return float(radius)


def mesh_curvature(scans, radius=0.1):
    """The functional form of DeviceScanSet.compute_curvature: computes the set's curvature with this radius unless it holds
    it already -> the per-scan list of (M_i,) float32 views into scans.curvature (zeros for a scan without a mesh)."""
    if not isinstance(scans, DeviceScanSet):
        raise ValueError("mesh_curvature: scans must be a DeviceScanSet")
    r = check_radius(radius, "mesh_curvature")
    if scans.curvature is None or scans.curvature_radius != r:
        scans.compute_curvature(r)
    return list(torch.split(scans.curvature, scans.sizes))


def check_curvature(scans, ids, who):
    """What curvatures=True needs of a batch's scans, on the host: ValueError before any device call."""
    if getattr(scans, "curvature", None) is None:
        raise ValueError("%s: curvatures=True needs the set's curvature -- call scans.compute_curvature() first (for a "
                         "FixMatchBatcher on both sets, with one radius, before it is built)" % who)
    for slot, i in enumerate(ids):
        if scans.has_mesh is None or not scans.has_mesh[int(i)]:
            raise ValueError("%s: batch slot %d (scan %d) has no mesh in this set: it has no curvature" % (who, slot, int(i)))


def curvature_sample(scans, ids_dev, sel_dev):
    """geot_curvature_sample, one launch on the current stream: ids_dev (S,) int64 scan numbers and sel_dev (S, m) int64 vertex
    indices local to each slot's scan, both on the device -> (curvatures (S, m) float32 = (|cur[sel]| - min) / (max - min)
    with the min and max of |cur| over the slot's WHOLE scan, 0 where max == min; bad (S,) int32: 1 where an index lies
    outside its scan (that entry is 0), 2 for a scan number outside the set)."""
    need(getattr(scans, "curvature", None) is not None, "curvature_sample: call scans.compute_curvature() first")
    dev = scans.device
    need(ids_dev.dtype == torch.int64 and ids_dev.device == dev and ids_dev.dim() == 1 and ids_dev.is_contiguous(),
         "curvature_sample: ids_dev must be a contiguous (S,) int64 tensor on %s" % dev)
    s = int(ids_dev.shape[0])
    need(sel_dev.dtype == torch.int64 and sel_dev.device == dev and sel_dev.dim() == 2 and sel_dev.is_contiguous() and
         sel_dev.shape[0] == s and sel_dev.shape[1] >= 1 and 1 <= s <= 65535,
         "curvature_sample: sel_dev must be a contiguous (S, m >= 1) int64 tensor on %s, 1 <= S <= 65535" % dev)
    out = torch.empty(tuple(sel_dev.shape), dtype=torch.float32, device=dev)
    bad = torch.empty(s, dtype=torch.int32, device=dev)
    call("geot_curvature_sample", dev, s, int(sel_dev.shape[1]), len(scans), int(scans.points.shape[0]), ptr(scans.curvature),
         ptr(scans._curvature_keys), ptr(scans.offsets), ptr(ids_dev), ptr(sel_dev), ptr(out), ptr(bad))
    return out, bad


def cloud_sample_batch(scans, scan_ids, sel, num_classes=17, check=True, ids_dev=None):
    """geot_cloud_sample_batch: scans a DeviceScanSet; scan_ids: the set scan of every batch slot (S ints, host); sel (S, m)
    int64 vertex indices local to each slot's scan (numpy or tensor) -> dict(raw (S, m, 3), y (S, m) int64, class_weights
    (S, num_classes), center (S, 3), scale (S,), bad (S,) int32).  Slot by slot bit-identical to prepare_sample on that scan
    alone; a slot flagged 2 (an unusable table entry: only the C entry point can be handed one, the ids are checked here)
    is zero-filled, class_weights included.  check=True reads `bad` back (one host sync) and raises IndexError for an index
    outside its scan.  ids_dev: scan_ids as an (S,) int64 tensor already on the device (the batchers upload them once for
    the draw and the sampling)."""
    need(isinstance(scans, DeviceScanSet), "cloud_sample_batch: scans must be a DeviceScanSet")
    ids = np.asarray(scan_ids, dtype=np.int64).reshape(-1)
    need(ids.size >= 1 and ids.min() >= 0 and ids.max() < len(scans), "cloud_sample_batch: scan ids must lie in [0, %d)" % len(scans))
    dev = scans.device
    if isinstance(sel, torch.Tensor):
        need(sel.dtype == torch.int64 and sel.dim() == 2, "sel must be (S, m) int64")
        sel_dev = sel.to(dev).contiguous()
    else:
        sel = np.ascontiguousarray(sel)
        need(sel.dtype == np.int64 and sel.ndim == 2, "sel must be (S, m) int64")
        sel_dev = _to_device(sel, dev)
    s, m = sel_dev.shape
    need(s == ids.size and m >= 1, "sel must have one row of m >= 1 indices per scan id")
    need(1 <= num_classes <= 4096, "num_classes must be in [1, 4096]")
    if ids_dev is None:
        ids_dev = _to_device(ids, dev)
    out = {"raw": torch.empty((s, m, 3), dtype=torch.float32, device=dev),
           "y": torch.empty((s, m), dtype=torch.int64, device=dev),
           "class_weights": torch.empty((s, num_classes), dtype=torch.float32, device=dev),
           "center": torch.empty((s, 3), dtype=torch.float32, device=dev),
           "scale": torch.empty(s, dtype=torch.float32, device=dev),
           "bad": torch.empty(s, dtype=torch.int32, device=dev)}
    nbytes = int(_lib.load().geot_cloud_sample_batch_ws_bytes(s, int(num_classes)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    call("geot_cloud_sample_batch", dev, s, m, int(num_classes), len(scans), int(scans.points.shape[0]), ptr(scans.points),
         ptr(scans.labels), ptr(scans.offsets), ptr(ids_dev), ptr(sel_dev), ptr(out["raw"]), ptr(out["y"]),
         ptr(out["class_weights"]), ptr(out["center"]), ptr(out["scale"]), ptr(out["bad"]), ptr(ws), nbytes)
    out["scan_ids"] = ids_dev
    if check:
        raise_bad_index(out["bad"], ids)
    return out


def raise_bad_index(bad, ids):
    flags = bad.cpu().numpy()            # the one host synchronisation of check=True
    if flags.any():
        slot = int(np.flatnonzero(flags)[0])
        raise IndexError("batch slot %d (scan %d): selected_idxs holds an index outside the scan" % (slot, int(ids[slot])))

