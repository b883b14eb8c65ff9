"""GPU suite: the eight channels-last pointops kernels of csrc/gather_group.hip (grouping, interpolation, subtraction,
aggregation and their gradients) through geot_amd/ext/pointops_cuda.py, each against its referee of tests/_gather_ref.py.

* grouping_cl, subtraction_cl and grad_position are one copy or one fp32 operation per element: exact, outputs pre-filled
  with NaN.
* interpolation_cl and aggregation_cl accumulate onto the caller's buffer, which arrives non-zero here: equal to the bit
  to the sequential fp32 loop in sample order starting from that value; the distance to the fp64 value is printed as a share
  of gamma(k + 1) resp. gamma(ns + 2) times the sum of absolute terms.
* the float-atomic gradients: fp64 scatter-add, gamma(n + 1) sum |terms| per element with n counted from the indices, and
  one integer-valued case each that must come out exact.
* the launch is capped at 8192 workgroups of 256 threads: WRAP shapes have 2 097 152 + 1024 elements, so the grid-stride
  loop's second trip runs; the sources of that trip have target rows of their own, which a missing trip would leave at zero.

Index sets: random with repeats, row 0 and the last row, a run of one value ("edges"); every index one hub; every index its
own row.

Measured on an MI355X, worst share of the bound over all cases (printed with -s); no kernel bug was found: the four exact
outputs and both fp32 restatements equal to the bit everywhere; interpolation_cl 0.590, aggregation_cl 0.532;
grouping_cl_grad 0.435, interpolation_cl_grad 0.555, subtraction_cl_grad 0.470 / 0.438, aggregation_cl_grad input 0.565,
weight 0.602; every integer-valued case exact.

Value-only faults planted in a scratch build, and what caught them: grouping_cl_kernel without its second trip -- the 1024
elements past 2 097 152 stay NaN in test_grid_stride_second_trip_forward alone; interpolation_cl_grad_kernel without it --
the tail rows stay 0 in test_grid_stride_second_trip_gradients alone; aggregation_cl_kernel starting from 0 instead of the
caller's value -- aggregation_cl in every case of test_forward and in the zero-samples test."""
import numpy as np
import pytest
import torch

import _gather_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

DEV = torch.device("cuda:0")
BASE = [(1, 1, 1, 1), (257, 3, 33, 11), (300, 8, 32, 8), (64, 16, 12, 1), (64, 5, 12, 12)]      # (n, ns, c, w_c)
KINDS = ("edges", "hub", "own row")
CAP = 8192 * 256                                  # elements the capped grid covers in one trip
WRAP3 = (2049, 16, 64)                            # (m, ns, c): outputs of m ns c elements
WRAP2 = (32784, 3, 64)                            # (n, k or ns, c): outputs of n c elements
TAIL_ROWS = 8                                     # target rows kept for the sources of the second trip


@pytest.fixture(scope="module")
def P():
    from geot_amd.ext import pointops_cuda
    return pointops_cuda


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def nans(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def zeros(*shape):
    return torch.zeros(shape, dtype=torch.float32, device=DEV)


def exact(got, want, label):
    bad = np.argwhere(~(got == want))
    assert not len(bad), (label, "first (index, got, want), count:", tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])], len(bad))


def share(got, want64, bound, label):
    err = np.abs(got.astype(np.float64) - want64)
    assert (err[bound == 0] == 0).all(), label
    s = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    assert s <= 1.0, (label, s)
    return s


def make_idx(rng, kind, n_in, shape):
    if kind == "hub":
        return np.full(shape, n_in // 2, np.int32)
    if kind == "own row":
        return np.ascontiguousarray(np.broadcast_to((np.arange(shape[0]) % n_in).astype(np.int32)[:, None], shape))
    return R.indices(rng, n_in, shape) if shape[0] * shape[1] else np.zeros(shape, np.int32)


def wrap_idx(rng, n_in, shape, c, by_row):
    """ids for a WRAP shape: the sources of the second trip draw from the last TAIL_ROWS rows of the input, every other one
    from the rows before them.  An element past CAP belongs to pair e / c of the flat (row, sample) list where the kernel
    has one lane per (row, sample, channel), and to row e / c (all its samples) where it has one lane per (row, channel)"""
    idx = rng.integers(0, n_in - TAIL_ROWS, shape).astype(np.int32)
    idx[0, 0], idx[1, 0] = 0, n_in - TAIL_ROWS - 1
    if by_row:
        idx[CAP // c:] = rng.integers(n_in - TAIL_ROWS, n_in, idx[CAP // c:].shape)
    else:
        flat = idx.reshape(-1)
        flat[CAP // c:] = rng.integers(n_in - TAIL_ROWS, n_in, flat.size - CAP // c)
    idx[-1, -1] = n_in - 1
    return idx


def inputs(tag, n, ns, c, w_c, kind, integer=False, n_in=None, idx=None):
    rng = R.rng_of("%s %d %d %d %d %s %d" % (tag, n, ns, c, w_c, kind, integer))
    n_in = n if n_in is None else n_in
    if idx is None:
        idx = make_idx(rng, kind, n_in, (n, ns))

    def draw(shape, lim):
        return (rng.integers(-lim, lim + 1, shape) if integer else rng.standard_normal(shape)).astype(np.float32)
    return {"idx": idx, "inp": draw((n_in, c), 4), "in1": draw((n, c), 4), "pos": draw((n, ns, c), 4),
            "w": draw((n, ns, w_c), 2), "wk": draw((n, ns), 2) if integer else R.weights(rng, (n, ns)),
            "out0": draw((n, c), 4), "g2": draw((n, c), 8), "g3": draw((n, ns, c), 8)}


# ---- launches ----------------------------------------------------------------------------------------------------------------

def run_forward(P, d):
    n, ns = d["idx"].shape
    c, w_c = d["inp"].shape[1], d["w"].shape[2]
    idx, inp = dev(d["idx"]), dev(d["inp"])
    grp, sub = nans(n, ns, c), nans(n, ns, c)
    itp, agg = dev(d["out0"]), dev(d["out0"])
    P.grouping_forward_cuda(n, ns, c, inp, idx, grp)
    P.subtraction_forward_cuda(n, ns, c, dev(d["in1"]), inp, idx, sub)
    P.interpolation_forward_cuda(n, c, ns, inp, idx, dev(d["wk"]), itp)
    P.aggregation_forward_cuda(n, ns, c, w_c, inp, dev(d["pos"]), dev(d["w"]), idx, agg)
    return host(grp), host(sub), host(itp), host(agg)


def check_forward(got, d, label):
    grp, sub, itp, agg = got
    exact(grp, R.grouping_cl_ref(d["inp"], d["idx"]), (label, "grouping_cl"))
    exact(sub, R.subtraction_cl_ref(d["in1"], d["inp"], d["idx"]), (label, "subtraction_cl"))
    exact(itp, R.interpolation_cl_ref32(d["inp"], d["idx"], d["wk"], d["out0"]), (label, "interpolation_cl"))
    exact(agg, R.aggregation_cl_ref32(d["inp"], d["pos"], d["w"], d["idx"], d["out0"]), (label, "aggregation_cl"))
    s1 = share(itp, *R.interpolation_cl_ref64(d["inp"], d["idx"], d["wk"], d["out0"]), (label, "interpolation_cl"))
    s2 = share(agg, *R.aggregation_cl_ref64(d["inp"], d["pos"], d["w"], d["idx"], d["out0"]), (label, "aggregation_cl"))
    print("forward %-40s share of the bound: interpolation_cl %.3f aggregation_cl %.3f" % (label, s1, s2))


def run_gradients(P, d):
    n, ns = d["idx"].shape
    n_in, c = d["inp"].shape
    w_c = d["w"].shape[2]
    idx, inp, pos, w = dev(d["idx"]), dev(d["inp"]), dev(d["pos"]), dev(d["w"])
    g_grp, g_itp, g_s1, g_s2 = zeros(n_in, c), zeros(n_in, c), zeros(n, c), zeros(n_in, c)
    g_in, g_pos, g_w = zeros(n_in, c), nans(n, ns, c), zeros(n, ns, w_c)
    P.grouping_backward_cuda(n, ns, c, dev(d["g3"]), idx, g_grp)
    P.interpolation_backward_cuda(n, c, ns, dev(d["g2"]), idx, dev(d["wk"]), g_itp)
    P.subtraction_backward_cuda(n, ns, c, idx, dev(d["g3"]), g_s1, g_s2)
    P.aggregation_backward_cuda(n, ns, c, w_c, inp, pos, w, idx, dev(d["g2"]), g_in, g_pos, g_w)
    return {"grouping_cl_grad": host(g_grp), "interpolation_cl_grad": host(g_itp), "subtraction_cl_grad in1": host(g_s1),
            "subtraction_cl_grad in2": host(g_s2), "aggregation_cl_grad input": host(g_in), "grad_position": host(g_pos),
            "aggregation_cl_grad weight": host(g_w)}


def gradient_referees(d):
    """name -> (fp64 value, bound), shaped as run_gradients' arrays; plus grad_position (fp32, exact)"""
    n, ns = d["idx"].shape
    n_in, c = d["inp"].shape
    w_c = d["w"].shape[2]
    g_pos, (r_in, t_in), (r_w, t_w) = R.aggregation_cl_grad_ref(d["inp"], d["pos"], d["w"], d["idx"], d["g2"])
    own = np.broadcast_to(np.arange(n)[:, None], (n, ns))
    ref = {"grouping_cl_grad": R.scatter_rows64(d["idx"], d["g3"], n_in),
           "interpolation_cl_grad": R.scatter_rows64(*R.interpolation_cl_grad_terms(d["g2"], d["idx"], d["wk"]), n_in),
           "subtraction_cl_grad in1": R.scatter_rows64(own, d["g3"], n),
           "subtraction_cl_grad in2": R.scatter_rows64(d["idx"], -d["g3"].astype(np.float64), n_in),
           "aggregation_cl_grad input": R.scatter_rows64(r_in, t_in, n_in),
           "aggregation_cl_grad weight": tuple(a.reshape(n, ns, w_c) for a in R.scatter_rows64(r_w, t_w, n * ns * w_c))}
    return ref, g_pos


def check_gradients(got, d, label, integer):
    ref, g_pos = gradient_referees(d)
    exact(got["grad_position"], g_pos, (label, "grad_position"))
    shares = {}
    for name, (want, bound) in ref.items():
        if integer:
            assert np.abs(want).max() < 2 ** 24
            exact(got[name], want.astype(np.float32), (label, name, "integer-valued"))
        else:
            shares[name] = share(got[name], want, bound, (label, name))
    if shares:
        print("gradients %-38s share of the bound: %s" % (label, ", ".join("%s %.3f" % kv for kv in shares.items())))


# ---- the tests ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,ns,c,w_c", BASE, ids=str)
def test_forward(P, n, ns, c, w_c, kind):
    d = inputs("fwd", n, ns, c, w_c, kind)
    check_forward(run_forward(P, d), d, "%s %s" % ((n, ns, c, w_c), kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,ns,c,w_c", BASE, ids=str)
def test_gradients(P, n, ns, c, w_c, kind):
    for integer in (False, True):
        d = inputs("grad", n, ns, c, w_c, kind, integer=integer)
        check_gradients(run_gradients(P, d), d, "%s %s" % ((n, ns, c, w_c), kind), integer)


def test_grouping_reads_a_table_of_another_length(P):
    """m output rows from n_in != m input rows, 0 and n_in - 1 among the ids"""
    d = inputs("grouping", 300, 8, 32, 8, "edges", n_in=41)
    m, ns, c = 300, 8, 32
    out, grad = nans(m, ns, c), zeros(41, c)
    P.grouping_forward_cuda(m, ns, c, dev(d["inp"]), dev(d["idx"]), out)
    P.grouping_backward_cuda(m, ns, c, dev(d["g3"]), dev(d["idx"]), grad)
    exact(host(out), R.grouping_cl_ref(d["inp"], d["idx"]), "grouping_cl")
    share(host(grad), *R.scatter_rows64(d["idx"], d["g3"], 41), "grouping_cl_grad")


def test_zero_samples_leave_the_buffers_as_they_came(P):
    n, c, w_c = 37, 12, 4
    rng = R.rng_of("zero")
    inp, out0 = rng.standard_normal((n, c)).astype(np.float32), rng.standard_normal((n, c)).astype(np.float32)
    e_i, e_f = torch.zeros((n, 0), dtype=torch.int32, device=DEV), zeros(n, 0)
    itp, agg, g1, g2, g3 = dev(out0), dev(out0), dev(out0), dev(out0), dev(out0)
    P.interpolation_forward_cuda(n, c, 0, dev(inp), e_i, e_f, itp)
    P.aggregation_forward_cuda(n, 0, c, w_c, dev(inp), zeros(n, 0, c), zeros(n, 0, w_c), e_i, agg)
    P.interpolation_backward_cuda(n, c, 0, dev(inp), e_i, e_f, g1)
    P.aggregation_backward_cuda(n, 0, c, w_c, dev(inp), zeros(n, 0, c), zeros(n, 0, w_c), e_i, dev(inp), g2, zeros(n, 0, c),
                                zeros(n, 0, w_c))
    P.grouping_backward_cuda(n, 0, c, zeros(n, 0, c), e_i, g3)
    for t in (itp, agg, g1, g2, g3):
        exact(host(t), out0, "zero samples")


def wrap_inputs(tag, shape, w_c, n_in, by_row):
    n, ns, c = shape
    rng = R.rng_of("wrap idx " + tag)
    return inputs(tag, n, ns, c, w_c, "wrap", n_in=n_in, idx=wrap_idx(rng, n_in, (n, ns), c, by_row))


def test_grid_stride_second_trip_forward(P):
    """2 097 152 + 1024 output elements per kernel; the elements past 2 097 152 are the second trip's"""
    for tag, shape in (("3-D", WRAP3), ("2-D", WRAP2)):
        n, ns, c = shape
        d = wrap_inputs(tag, shape, 8, 1000, tag == "2-D")
        grp, sub, itp, agg = run_forward(P, d)
        if tag == "3-D":                          # grouping, subtraction: n ns c elements
            assert grp.size == sub.size == CAP + 1024
            want_g, want_s = R.grouping_cl_ref(d["inp"], d["idx"]), R.subtraction_cl_ref(d["in1"], d["inp"], d["idx"])
            exact(grp.reshape(-1)[CAP:], want_g.reshape(-1)[CAP:], "grouping_cl, second trip")
            exact(sub.reshape(-1)[CAP:], want_s.reshape(-1)[CAP:], "subtraction_cl, second trip")
            exact(grp, want_g, "grouping_cl")
            exact(sub, want_s, "subtraction_cl")
        else:                                     # interpolation, aggregation: n c elements
            assert itp.size == agg.size == CAP + 1024
            want_i = R.interpolation_cl_ref32(d["inp"], d["idx"], d["wk"], d["out0"])
            want_a = R.aggregation_cl_ref32(d["inp"], d["pos"], d["w"], d["idx"], d["out0"])
            exact(itp.reshape(-1)[CAP:], want_i.reshape(-1)[CAP:], "interpolation_cl, second trip")
            exact(agg.reshape(-1)[CAP:], want_a.reshape(-1)[CAP:], "aggregation_cl, second trip")
            exact(itp, want_i, "interpolation_cl")
            exact(agg, want_a, "aggregation_cl")


def test_grid_stride_second_trip_gradients(P):
    """the sources past 2 097 152 elements scatter to the last TAIL_ROWS input rows, which nothing else touches: a missing
    second trip leaves them (and the tail of the outputs indexed by the source itself) at zero, far outside the bound"""
    for tag, shape, names in (("3-D", WRAP3, ("grouping_cl_grad", "subtraction_cl_grad in1", "subtraction_cl_grad in2")),
                              ("2-D", WRAP2, ("interpolation_cl_grad", "aggregation_cl_grad input", "aggregation_cl_grad weight"))):
        n, ns, c = shape
        d = wrap_inputs(tag + " grad", shape, 8, 1000, tag == "2-D")
        got = run_gradients(P, d)
        ref, g_pos = gradient_referees(d)
        if tag == "2-D":
            exact(got["grad_position"][CAP // c:], g_pos[CAP // c:], "grad_position, second trip")
            exact(got["grad_position"], g_pos, "grad_position")
        for name in names:
            want, bound = ref[name]
            s = share(got[name], want, bound, (tag, name))
            by_source = name in ("subtraction_cl_grad in1", "aggregation_cl_grad weight")
            tail = want[CAP // c // (ns if tag == "3-D" else 1):] if by_source else want[-TAIL_ROWS:]
            assert tail.size and (np.abs(tail) > 100 * bound.max()).any(), (tag, name)     # zero there would miss the bound
            print("second trip %-28s share of the bound %.3f" % (name, s))
