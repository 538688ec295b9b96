"""Every launch form of the rows GEMM (csrc/rows_gemm.hip) and of the weight gradient (csrc/wgrad.hip), pinned by the library's
launch-form counters (tdnnf_gemm_launch_forms) and compared ELEMENT BY ELEMENT with a float64 product formed on the GPU.

Each case resets the counters, calls a public entry, asserts that exactly the intended (tile, arithmetic, form) counters moved and
holds every output element to a derived bound.  The shapes are worked out by hand from the planner's rules for a chip of 256 compute
units; on another chip the shape-specific cases skip.  The counter is the judge: a case whose shape stops landing on its form fails.

Bounds (u = 2^-24, the unit roundoff of float32; mag = (|A| |B|)_ij plus the magnitudes of the epilogue's terms, all in float64):
  exact f32   |C - C64| <= (K + S + c) u mag   for ANY order of the K products' float32 summation in S slices that a float32 pass adds;
              c = 4 covers the epilogue (bias or the value added into, the learning-rate scale) and the second-order terms of
              K u / (1 - K u) at these K.  Two forms of one arithmetic therefore agree within twice that.
  bf16x3      operands are the sum of two bf16 planes, each the round-to-nearest of what is left (csrc/gemm_dev.h split_bf16): the
              planes leave |x - p0 - p1| <= 2^-16 |x|, the product drops p1 q1 <= 2^-16 (1 + 2^-7) |x y|, so one product errs by at
              most 3 * 2^-16 * (1 + 2^-6) |x y|; the three kept products per k are exact in float32 and summed in float32:
              |C - C64| <= (3 * 2^-16 (1 + 2^-6) + (3 K + S + c) u) mag.
  bf16x6      three planes leave 2^-24 |x|; dropped are p1 q2, p2 q1 (2^-24 each) and p2 q2: one product errs by at most
              (4 * 2^-24 + 2^-32)(1 + 2^-6) |x y|, six products per k: |C - C64| <= (4.1 * 2^-24 + (6 K + S + c) u) mag.
No bound here is taken from the output of the code under test.  For the record, the worst |err| / bound over all cases measured on an
MI355X (every case prints its own): exact f32 0.032 (rows GEMM; K = 160 .. 256), 0.026 (weight gradient, 200 rows); bf16x3 0.032
(plain, K = 108), 0.026 (main + tail); bf16x6 0.0032.  The errors behave like sqrt(K) u, the bounds are the worst case K u; a dropped
K step, a row read one off or a wrong scratch pitch is an error of the size of mag itself.

The ||row||^2 by-product of the statistics passes: one entry per 128-row block without the K split, compared block by block; with the split
only the total is defined by the C-ABI.  Both to (K + 4) u relative, derived at the assertion."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.gpu_util import Hip
from tests.view_layouts import laid_out

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
EPS = {"f32": 0.0, "bf16x3": 3 * 2.0 ** -16 * (1 + 2.0 ** -6), "bf16x6": 4.1 * 2.0 ** -24}
PRODUCTS = {"f32": 1, "bf16x3": 3, "bf16x6": 6}
ARITH_OPTION = {"f32": 0, "bf16x3": 1, "bf16x6": 3}


@pytest.fixture(scope="module")
def hip(pkg):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return Hip(pkg)


@pytest.fixture
def cus256():
    n = torch.cuda.get_device_properties(0).multi_processor_count
    if n != 256:
        pytest.skip("the shapes of this case are derived for 256 compute units, the device reports %d" % n)


def bound(mag, K, S=1, arith="f32", c=4):
    return (EPS[arith] + (PRODUCTS[arith] * K + S + c) * U) * mag


def assert_within(got, ref, bnd, what):
    """every element of got (float32, device) within bnd of ref (float64, device); prints the worst ratio err / bound"""
    err = (got.double() - ref).abs()
    assert bool(torch.isfinite(got).all()), what
    ratio = float((err / bnd.clamp_min(1e-300)).max())
    print("%s: worst |err| / bound = %.3g" % (what, ratio))
    bad = (err > bnd).nonzero()
    assert bad.numel() == 0, "%s: %d elements over the bound, first %s, worst err / bound %.3g" % (what, bad.shape[0], bad[0].tolist(), ratio)


class options:
    """several tuning options for the duration of a block"""

    def __init__(self, pkg, **kw):
        self.ctx = [pkg.hipabi.option(k, v) for k, v in kw.items()]

    def __enter__(self):
        for c in self.ctx:
            c.__enter__()

    def __exit__(self, *exc):
        for c in reversed(self.ctx):
            c.__exit__(*exc)
        return False


def forms(pkg):
    """the form counters that moved since the last reset; apart from them the two gauges and the vec4 / scalar launch counts"""
    f = pkg.hipabi.launch_forms(reset=True)
    gauges = {k: f.pop(k) for k in ("rows.last_slices", "wgrad.last_slabs", "rows.launches_vec4", "rows.launches_scalar") if k in f}
    return f, gauges


def assert_loads(g, scalar):
    """every rows GEMM kernel of the call loaded float by float (scalar) / 16 bytes at a time"""
    want, other = ("rows.launches_scalar", "rows.launches_vec4") if scalar else ("rows.launches_vec4", "rows.launches_scalar")
    assert g.get(want, 0) >= 1 and other not in g, g


# ---------------------------------------------------------------------------------------------------------------- rows GEMM, forward
class Prop:
    """One tdnn_propagate problem: out (M x Do) = sum over taps i of X[off_i + rho m] W_i^T, its float64 value and magnitude."""

    def __init__(self, M, Do, Di, offs=(0,), rho=1, seed=0, x_layout=None, w_pad=False):
        g = torch.Generator(device="cuda").manual_seed(1000 + seed)
        self.M, self.Do, self.Di, self.offs, self.rho, self.K = M, Do, Di, tuple(offs), rho, len(offs)
        rows_in = (M - 1) * rho + max(offs) + 1
        x = torch.randn(rows_in, Di, generator=g, device="cuda")
        W = torch.randn(Do, self.K * Di, generator=g, device="cuda") / float(np.sqrt(self.K * Di))
        self.bias = torch.randn(Do, generator=g, device="cuda")
        self.y0 = torch.randn(M, Do, generator=g, device="cuda")
        if x_layout is None:
            self.x = _padded_dev(x, float("nan"))  # (what lies beside the matrix must never reach a product)
            self.check_x = lambda: None
        else:
            self.x, _, self.check_x = laid_out(x.cpu().numpy(), x_layout)
        self.ldw = self.K * Di
        if w_pad:  # a weight matrix with 16-byte aligned rows whatever K Di is
            self.ldw = (self.K * Di + 3) // 4 * 4 + 4
            wb = torch.full((Do, self.ldw), float("nan"), device="cuda")
            wb[:, :self.K * Di] = W
            self.W = wb
        else:
            self.W = W.contiguous()
        rows = torch.arange(M, device="cuda") * rho
        self.ref = torch.zeros(M, Do, dtype=torch.float64, device="cuda")
        self.mag = torch.zeros(M, Do, dtype=torch.float64, device="cuda")
        for i, o in enumerate(offs):
            xi, wi = x[rows + o].double(), W[:, i * Di:(i + 1) * Di].double()
            self.ref += xi @ wi.T
            self.mag += xi.abs() @ wi.abs().T
        self.ktot = self.K * Di

    def run(self, hip, pkg, mode=2, out_layout=None):
        """(got, want, magnitude) of one call with init_mode `mode`; the output's surroundings are checked"""
        ix = pkg.hipabi.indexes(self.rho, self.offs)
        if out_layout is None:
            yd, ybuf = _padded_pair(self.y0, 7.0)
            check = lambda: _assert_pad_untouched(ybuf, self.Do, 7.0)
        else:
            yd, _, check = laid_out(self.y0.cpu().numpy(), out_layout, writes=True)
        hip.tdnn_propagate(C.byref(ix), self.x, hip.vec(self.W), self.ldw, self.Do, self.Di, hip.vec(self.bias) if mode == 1 else None, None, mode, yd,
                           hip.stream())
        torch.cuda.synchronize()
        check()
        self.check_x()
        extra = self.bias.double() if mode == 1 else self.y0.double() if mode == 0 else None
        want = self.ref if extra is None else self.ref + extra
        mag = self.mag if extra is None else self.mag + extra.abs()
        return yd, want, mag


def _padded_dev(t, fill):
    return _padded_pair(t, fill)[0]


def _padded_pair(t, fill):
    """gpu_util.padded() for a device tensor: the view and its wider buffer"""
    stride = (t.shape[1] + 3) // 4 * 4 + 4
    buf = torch.full((t.shape[0], stride), fill, dtype=torch.float32, device="cuda")
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]], buf


def _assert_pad_untouched(buf, cols, fill):
    assert bool((buf[:, cols:] == fill).all()), "wrote outside the view"


def check_prop(hip, pkg, p, want_forms, S, arith="f32", modes=(2,), slices=None, out_layout=None, what="", scalar=False):
    outs = []
    for mode in modes:
        forms(pkg)
        got, want, mag = p.run(hip, pkg, mode, out_layout)
        f, g = forms(pkg)
        assert f == want_forms, (what, mode, f)
        assert_loads(g, scalar)
        if slices is not None:
            assert g.get("rows.last_slices") == slices, (what, g)  # (the scratch of a split launch is sized for the planned slices)
        assert_within(got, want, bound(mag, p.ktot, S, arith), "%s mode %d %s" % (what, mode, sorted(want_forms)))
        outs.append(got)
    return outs


def one(tile, form, arith="f32", **more):
    d = {"rows.%s.%s.%s" % (tile, arith, form): 1}
    d.update(more)
    return d


def test_counter_names_are_unique_and_reset(pkg):
    lib = pkg.hipabi.load()
    n = lib.tdnnf_gemm_launch_forms(None, 0, 1)
    names = [lib.tdnnf_gemm_launch_form_name(i).decode() for i in range(n)]
    assert len(set(names)) == n and lib.tdnnf_gemm_launch_form_name(n) is None and lib.tdnnf_gemm_launch_form_name(-1) is None
    assert "rows.64x128k16.f32.partial_s2" in names and "planes.main_split_tail" in names and "wgrad.64x64.f32" in names
    assert pkg.hipabi.launch_forms() == {}


def test_plain_64x128(hip, pkg, cus256):
    """15 x 50, three taps of 36: one ragged tile, a reduction below 256, nothing splits"""
    check_prop(hip, pkg, Prop(15, 50, 36, (0, 2, 3), seed=1), one("64x128k16", "plain"), 1, modes=(1, 0, 2), what="plain")


@pytest.mark.parametrize("per_cu", [2, 1])
@pytest.mark.parametrize("shape", ["threshold", "ragged"])
def test_whole_launch_split_k_64x128(hip, pkg, cus256, shape, per_cu):
    """one tile with K = 256, the shortest reduction that splits (16 K steps, 4 slices of 4), and 70 x 50 with one tap of 301: a
    reduction that is no multiple of 4, an output width that is none either (the partial tiles' pitch), a ragged last slice
    (19 K steps: slices of 5 steps = 80, the last 61 long)"""
    p = Prop(64, 128, 256, seed=2) if shape == "threshold" else Prop(70, 50, 301, seed=3, w_pad=True)
    with options(pkg, splitk_per_cu=per_cu):
        check_prop(hip, pkg, p, one("64x128k16", "splitk"), 4, modes=(1, 0, 2), slices=4, what="splitk " + shape)


def test_split_k_slices_per_cu(hip, pkg, cus256):
    """option splitk_per_cu at a shape where it decides: 2 560 x 128 with K = 1 024 is 40 tiles of 64 x 128 and 64 K steps.  The default fills
    the 1 024 slots (25 slices per tile, capped at 64 / 4 = 16 slices of 4 steps); value 1 asks for one slice per CU, 256 / 40 = 6 slices of
    ceil(64 / 6) = 11 steps.  Both hold the bound, and they agree within the sum of their bounds."""
    p = Prop(2560, 128, 1024, seed=19)
    out = {}
    for per_cu, S in ((2, 16), (1, 6)):
        with options(pkg, splitk_per_cu=per_cu):
            out[per_cu], = check_prop(hip, pkg, p, one("64x128k16", "splitk"), S, modes=(1,), slices=S, what="splitk_per_cu %d" % per_cu)
    mag = p.mag + p.bias.double().abs()
    assert not torch.equal(out[1], out[2])  # (other slices, another summation order)
    assert_within(out[1], out[2].double(), bound(mag, p.ktot, 16) + bound(mag, p.ktot, 6), "one slice per CU against two")


PARTIAL = {
    # name: (M, Do, Di, offsets, tile, form, S)        19 200 rows: 300 tiles of 64 on 1 024 slots, 48 K steps -> S = 2
    "64x128-s2": (19200, 128, 384, (0, 1), "64x128k16", "partial_s2", 2),
    # one row tile over / at the threshold tiles * 4 > slots: 257 tiles split by 2, 256 tiles take the whole-launch split (S = 4)
    "64x128-257-tiles": (16385, 128, 384, (0, 1), "64x128k16", "partial_s2", 2),
    "64x128-256-tiles": (16384, 128, 384, (0, 1), "64x128k16", "splitk", 4),
    # 188 tiles of 128 x 160 on 512 slots, 96 K steps -> S = 4 (the source's own example); 129 tiles -> S = 3; 128 tiles: whole-launch split
    "128x160-s4": (24064, 160, 1536, (0,), "128x160k16", "partial_s4", 4),
    "128x160-129-tiles": (16385, 160, 1536, (0,), "128x160k16", "partial_s3", 3),
    "128x160-128-tiles": (16384, 160, 1536, (0,), "128x160k16", "splitk", 4),
}


@pytest.mark.parametrize("name", sorted(PARTIAL))
def test_partial_round_split_k(hip, pkg, cus256, name):
    M, Do, Di, offs, tile, form, S = PARTIAL[name]
    p = Prop(M, Do, Di, offs, seed=4)
    got, = check_prop(hip, pkg, p, one(tile, form), S, modes=(0,), slices=S, what=name)
    if form.startswith("partial"):  # the same call with the option off: a plain launch, the same bound, and the two agree
        with options(pkg, splitk_partial_round=0):
            plain, = check_prop(hip, pkg, p, one(tile, "plain"), 1, modes=(0,), what=name + " option off")
        mag = p.mag + p.y0.double().abs()
        assert_within(got, plain.double(), bound(mag, p.ktot, S) + bound(mag, p.ktot, 1), name + " against plain")


TAILS = {
    # name: (M, Do, Di, tile, K slices of the tail, rows of the main launch)
    # 76 x 12 = 912 tiles on 768 slots: 64 whole tile rows, then 1 536 rows as 144 tiles in 5 slices of 14 K steps
    "k16": (9728, 1536, 220, "128x128k16", 5, 8192),
    # the tail's last row tile ragged, the width no multiple of 4
    "k16-ragged-rows-odd-width": (9700, 1534, 220, "128x128k16", 5, 8192),
    # 86 x 12 = 1 032 tiles on 512 slots: two rounds and 8 tiles; the tail one ragged row tile (12 tiles), 17 K steps of 32 in slices of
    # ceil(17 / 8) = 3 steps: 6 slices
    "k32": (10958, 1536, 520, "128x128k32", 6, 10880),
}


@pytest.mark.parametrize("name", sorted(TAILS))
def test_main_launch_and_split_k_tail(hip, pkg, cus256, name):
    """(K = 220 / 520 are no multiples of 16, so the main launch is the tile kernel, not the ring)"""
    M, Do, Di, tile, S, m_main = TAILS[name]
    p = Prop(M, Do, Di, seed=5)
    forms(pkg)
    got, want, mag = p.run(hip, pkg, 1)
    f, g = forms(pkg)
    assert f == one(tile, "main_split_tail", **{"rows.%s.f32.plain" % tile: 1}), f
    assert g.get("rows.last_slices") == S, g
    # main rows and tail rows on their own, so that a tail error cannot hide in the whole
    assert_within(got[:m_main], want[:m_main], bound(mag[:m_main], p.ktot, 1), name + " main rows")
    assert_within(got[m_main:], want[m_main:], bound(mag[m_main:], p.ktot, S), name + " tail rows")


def test_main_launch_and_ring_main(hip, pkg, cus256):
    """the same split with whole K steps (K = 224): the main launch is the ring's"""
    p = Prop(9728, 1536, 224, seed=6)
    forms(pkg)
    got, want, mag = p.run(hip, pkg, 0)
    f, _ = forms(pkg)
    assert f == {"rows.128x128k16.f32.main_split_tail": 1, "rows.128x128k16.f32.ring": 1}, f
    assert_within(got[:8192], want[:8192], bound(mag[:8192], p.ktot, 1), "ring main rows")
    assert_within(got[8192:], want[8192:], bound(mag[8192:], p.ktot, 5), "tail rows")


def test_main_launch_and_plain_tail(hip, pkg, cus256):
    """230 x 5 = 1 150 tiles on 768 slots: 153 whole tile rows (765 tiles; 768 is no multiple of 5), then 77 tile rows = 385 tiles, more than
    half the slots, so nothing to split: two plain launches"""
    p = Prop(29440, 640, 200, seed=7)
    forms(pkg)
    got, want, mag = p.run(hip, pkg, 1)
    f, _ = forms(pkg)
    assert f == {"rows.128x128k16.f32.main_plain_tail": 1, "rows.128x128k16.f32.plain": 2}, f
    m_main = 153 * 128
    assert_within(got[:m_main], want[:m_main], bound(mag[:m_main], p.ktot), "main rows")
    assert_within(got[m_main:], want[m_main:], bound(mag[m_main:], p.ktot), "tail rows")


@pytest.mark.parametrize("M,tile", [(1024, "128x32k32"), (1023, "64x128k16"), (1101, "128x32k32")])
def test_skinny_outputs(hip, pkg, cus256, M, tile):
    """at most 32 columns: the 128 x 32 tile from 1 024 rows on, below that the tile of any small launch"""
    check_prop(hip, pkg, Prop(M, 20, 100, seed=8), one(tile, "plain"), 1, modes=(1, 0), what="skinny %d" % M)


@pytest.mark.parametrize("form", ["plain", "splitk"])
def test_scalar_kernels(hip, pkg, cus256, form):
    """the input 4 bytes off 16-byte alignment: the kernels that load float by float; the output in a guarded view"""
    p = Prop(15, 50, 36, (0, 2, 3), seed=9, x_layout="off1") if form == "plain" else Prop(70, 50, 301, seed=10, x_layout="off1")
    check_prop(hip, pkg, p, one("64x128k16", form), 1 if form == "plain" else 4, modes=(1, 0), out_layout="off1", what="scalar " + form, scalar=True)


@pytest.mark.parametrize("offs,rho", [((0, 1), 1), ((0, 3), 3)])
def test_two_taps_of_one_matrix(hip, pkg, cus256, offs, rho):
    """300 rows: five row tiles of 64, the last ragged; odd tiles visit the taps in reverse order with gemm_alt_taps 1"""
    p = Prop(300, 128, 64, offs, rho, seed=11)
    out = {}
    for alt in (0, 1):
        with options(pkg, gemm_alt_taps=alt):
            out[alt], = check_prop(hip, pkg, p, one("64x128k16", "plain"), 1, modes=(1,), what="two taps, alt %d" % alt)
    mag = p.mag + p.bias.double().abs()
    assert_within(out[1], out[0].double(), 2 * bound(mag, p.ktot), "alt order against tap order")


RING = {
    # 12 x 97 = 1 164 tiles on 768 slots (396 left over: more than half a round, no tail): ragged last row tile (91 rows) and column tile (72)
    "k2": (1499, 12360, 160, (0, 1), 1, (1, 0, 2)),
    "k2-stride3": (1499, 12360, 160, (0, 3), 3, (2,)),
}


@pytest.mark.parametrize("name", sorted(RING))
def test_persistent_ring(hip, pkg, cus256, name):
    M, Do, Di, offs, rho, modes = RING[name]
    p = Prop(M, Do, Di, offs, rho, seed=12)
    ring = check_prop(hip, pkg, p, one("128x128k16", "ring"), 1, modes=modes, what="ring " + name)
    with options(pkg, gemm_ring=0):
        plain = check_prop(hip, pkg, p, one("128x128k16", "plain"), 1, modes=modes[:1], what="ring off " + name)
    mag = p.mag + (p.bias.double().abs() if modes[0] == 1 else 0)
    assert_within(ring[0], plain[0].double(), 2 * bound(mag, p.ktot), "ring against tile kernel")


def test_persistent_ring_on_the_160_tile(hip, pkg, cus256):
    """gemm_ring 2: 1 000 x 300 on 128 x 160 tiles (ragged rows, a 140-column tile), K = 160 (too short to split)"""
    p = Prop(1000, 300, 160, seed=13)
    check_prop(hip, pkg, p, one("128x160k16", "plain"), 1, modes=(1,), what="160 tile, ring 1")
    with options(pkg, gemm_ring=2):
        check_prop(hip, pkg, p, one("128x160k16", "ring"), 1, modes=(1, 0, 2), what="160 tile, ring 2")


# ---------------------------------------------------------------------------------------------------- the in-kernel split arithmetics
SPLIT_TILE = {"bf16x3": "128x128k32", "bf16x6": "128x128k16"}


@pytest.mark.parametrize("arith", ["bf16x3", "bf16x6"])
@pytest.mark.parametrize("form", ["plain", "splitk", "partial", "main_split_tail", "misaligned"])
def test_split_arithmetics(hip, pkg, cus256, arith, form):
    """option gemm_arith_test: the stand-alone entry on the bf16x3 / bf16x6 kernels (k-contiguous weights, 16-byte aligned operands)"""
    tile = SPLIT_TILE[arith]
    with options(pkg, gemm_arith_test=ARITH_OPTION[arith]):
        if form == "plain":
            check_prop(hip, pkg, Prop(15, 50, 36, (0, 2, 3), seed=14), one(tile, "plain", arith), 1, arith, modes=(1, 0, 2), what=arith + " plain")
        elif form == "splitk":  # K = 512: 16 steps of 32 -> 4 slices, 32 steps of 16 -> 8
            S = 4 if arith == "bf16x3" else 8
            check_prop(hip, pkg, Prop(70, 50, 512, seed=15), one(tile, "splitk", arith), S, arith, modes=(1, 0), slices=S, what=arith + " splitk")
        elif form == "partial":  # 188 tiles of 128 x 160 on 512 (256) slots
            check_prop(hip, pkg, Prop(24064, 160, 1536, seed=16), one("128x160k16", "partial_s4", arith), 4, arith, modes=(0,), slices=4, what=arith + " partial")
        elif form == "main_split_tail":  # 1 032 tiles on 512 slots; the tail's 12 tiles in 4 slices of 2 K steps of 32, 8 of 2 steps of 16
            p = Prop(10958, 1536, 256, seed=17)
            S = 4 if arith == "bf16x3" else 8
            forms(pkg)
            got, want, mag = p.run(hip, pkg, 1)
            f, g = forms(pkg)
            assert f == one(tile, "main_split_tail", arith, **{"rows.%s.%s.plain" % (tile, arith): 1}), f
            assert g.get("rows.last_slices") == S, g
            assert_within(got[:10880], want[:10880], bound(mag[:10880], p.ktot, 1, arith), arith + " main rows")
            assert_within(got[10880:], want[10880:], bound(mag[10880:], p.ktot, S, arith), arith + " tail rows")
        else:  # an operand off alignment: exact f32, and held to ITS bound
            check_prop(hip, pkg, Prop(15, 50, 36, (0, 2, 3), seed=18, x_layout="off1"), one("64x128k16", "plain"), 1, "f32", modes=(1,), what=arith + " misaligned",
                       scalar=True)


# ------------------------------------------------------------------------------------------------- rows GEMM, backward (B not k-contiguous)
BACKPROP = {
    # name: (N rows of out_deriv, Do = reduction per tap, Di = output width, offsets, form, S)
    "plain": (15, 108, 50, (0,), "plain", 1),
    "splitk": (64, 256, 128, (0,), "splitk", 4),
    "partial": (19199, 384, 128, (0, 1), "partial_s2", 2),  # 19 200 rows of in_deriv
}


@pytest.mark.parametrize("name", sorted(BACKPROP))
def test_backprop_data_forms(hip, pkg, cus256, name):
    """tdnn_backprop_data: the output derivative is the A operand, W is read as B[k][n], the result adds into a non-zero in_deriv"""
    N, Do, Di, offs, form, S = BACKPROP[name]
    g = torch.Generator(device="cuda").manual_seed(77)
    K = len(offs)
    rows_in = N + max(offs)
    dy = torch.randn(N, Do, generator=g, device="cuda")
    W = (torch.randn(Do, K * Di, generator=g, device="cuda") / float(np.sqrt(K * Do))).contiguous()
    dx0 = torch.randn(rows_in, Di, generator=g, device="cuda")
    ref, mag = dx0.double().clone(), dx0.double().abs()
    for i, o in enumerate(offs):
        wi = W[:, i * Di:(i + 1) * Di].double()
        ref[o:o + N] += dy.double() @ wi
        mag[o:o + N] += dy.double().abs() @ wi.abs()
    ix = pkg.hipabi.indexes(1, offs)
    dyd = _padded_dev(dy, float("nan"))
    dxd, dxbuf = _padded_pair(dx0, 7.0)
    forms(pkg)
    hip.tdnn_backprop_data(C.byref(ix), dyd, hip.vec(W), K * Di, Do, Di, None, dxd, hip.stream())
    torch.cuda.synchronize()
    f, gz = forms(pkg)
    assert f == one("64x128k16", form), f
    if S > 1:
        assert gz.get("rows.last_slices") == S, gz
    _assert_pad_untouched(dxbuf, Di, 7.0)
    assert_within(dxd, ref, bound(mag, K * Do, S), "backprop " + name)


# ------------------------------------------------------------------------------------------------------------ the statistics passes
NG = {
    # name: (rank, Di, ng_bk, tile)
    "rank20": (20, 1024, 0, "128x32k32"),
    "rank20-bk1": (20, 1024, 1, "128x32k64"),
    "rank40": (40, 1024, 0, "128x64k32"),
    "rank40-bk8": (40, 1024, 8, "128x96k16"),
    "rank80": (80, 1024, 0, "128x96k16"),
    "rank80-bk2": (80, 1024, 2, "128x96k32"),
    "rank80-bk4": (80, 1024, 4, "128x128k32"),
    "rank80-long": (80, 2048, 0, "128x128k32"),
    # the bits that are not a rank's own leave its tile alone
    "rank20-bk14": (20, 1024, 2 | 4 | 8, "128x32k32"),
    "rank40-bk7": (40, 1024, 1 | 2 | 4, "128x64k32"),
    "rank80-bk9": (80, 1024, 1 | 8, "128x96k16"),
    "rank80-long-bk6": (80, 2048, 2 | 4, "128x128k32"),
}


@pytest.mark.parametrize("rows", [700, 16500], ids=["split", "whole"])
@pytest.mark.parametrize("name", sorted(NG))
def test_statistics_pass_forms(hip, pkg, cus256, name, rows):
    """tdnnf_ng_stats_pass on the MFMA rows GEMM: 700 rows are 6 row tiles (4 x 6 <= 512 slots: K splits over the idle CUs, at most 16
    slices of at least 4 K steps), 16 500 rows are 129 (no split)"""
    R, Di, bk, tile = NG[name]
    g = torch.Generator(device="cuda").manual_seed(R + rows)
    X = torch.randn(rows, Di, generator=g, device="cuda")
    W = torch.randn(R, Di, generator=g, device="cuda") / float(np.sqrt(Di))
    xd = _padded_dev(X, float("nan"))
    ldw = Di
    ref, mag = X.double() @ W.double().T, X.double().abs() @ W.double().abs().T
    sq = float(X.double().pow(2).sum())
    cap = 1024
    H, hbuf = _padded_pair(torch.full((rows, R), float("nan"), device="cuda"), 7.0)
    part = torch.full((cap,), float("nan"), dtype=torch.float64, device="cuda")
    ix = pkg.hipabi.indexes(1, (0,))
    forms(pkg)
    with options(pkg, ng_bk=bk):
        hip.ng_stats_pass(C.byref(ix), xd, Di, None, None, hip.vec(W.contiguous()), ldw, None, H, hip.vec(part), cap, 0, None, 0, hip.stream())
    torch.cuda.synchronize()
    f, gz = forms(pkg)
    split = rows == 700
    assert f == one(tile, "sumsq_splitk" if split else "sumsq_plain"), f
    S = gz.get("rows.last_slices", 1) if split else 1
    assert not split or 2 <= S <= 16, gz
    _assert_pad_untouched(hbuf, R, 7.0)
    assert_loads(gz, False)
    assert_within(H, ref, bound(mag, Di, S), "statistics pass " + name)
    # ||row||^2: each of a block's 256 threads adds the squares it stages in float32 -- 128 rows x K / 256 threads = K / 2 positive terms,
    # each square rounded once -- and the threads' sums are added in double: relative error at most (K / 2 + 1) u per entry, held to
    # (K + 4) u.  Without the K split entry b is the sum over rows [128 b, 128 b + 128), compared block by block; with it the entries are
    # (block, slice) sums in an order the C-ABI does not fix, so their total is compared, to the same relative bound (all terms positive).
    rel = (Di + 4) * U
    if not split:
        blocks = (rows + 127) // 128
        rowsq = torch.zeros(blocks * 128, dtype=torch.float64, device="cuda")
        rowsq[:rows] = X.double().pow(2).sum(1)
        want_b = rowsq.view(blocks, 128).sum(1)
        assert_within(part[:blocks], want_b, rel * want_b, "statistics pass %s, ||row||^2 per block" % name)
        assert not bool(part[blocks:].any()), "entries no block owns must be zero"
    assert abs(float(part.sum()) - sq) <= rel * sq, (float(part.sum()), sq)


# ------------------------------------------------------------------------------------------------------------------ weight gradient
WGRAD = {
    # name: (Do, Di, counter tile)
    "32x128": (20, 200, "32x128"),
    "160x128": (160, 96, "160x128"),
    "128x160": (256, 160, "128x160"),
    "128x128": (200, 120, "128x128"),
}


def _wgrad_case(hip, pkg, Do, Di, K, N, tile, slabs=None):
    g = torch.Generator(device="cuda").manual_seed(Do + Di + N)
    offs = tuple(range(K))
    X = torch.randn(N + K - 1, Di, generator=g, device="cuda")
    dY = torch.randn(N, Do, generator=g, device="cuda")
    W0 = torch.randn(Do, K * Di, generator=g, device="cuda")
    b0 = torch.randn(Do, generator=g, device="cuda")
    lr = 0.5
    ref, mag = W0.double().clone(), W0.double().abs()
    for i, o in enumerate(offs):
        ref[:, i * Di:(i + 1) * Di] += lr * (dY.double().T @ X[o:o + N].double())
        mag[:, i * Di:(i + 1) * Di] += lr * (dY.double().abs().T @ X[o:o + N].double().abs())
    bref, bmag = b0.double() + lr * dY.double().sum(0), b0.double().abs() + lr * dY.double().abs().sum(0)
    xd, dyd = _padded_dev(X, float("nan")), _padded_dev(dY, float("nan"))
    Wacc, wbuf = _padded_pair(W0, 7.0)
    bacc = b0.clone()
    nbytes = hip.tdnn_update_workspace_bytes(Do, Di, K, N)
    ws = hip.ws(nbytes)
    ix = pkg.hipabi.indexes(1, offs)
    forms(pkg)
    hip.tdnn_update_simple(C.byref(ix), xd, dyd, Do, Di, None, lr, hip.vec(Wacc), wbuf.stride(0), hip.vec(bacc), hip.vec(ws), nbytes, hip.stream())
    torch.cuda.synchronize()
    f, gz = forms(pkg)
    assert f == {"wgrad.%s.f32" % tile: 1}, f
    S = gz["wgrad.last_slabs"]
    if slabs is not None:
        assert S == slabs, gz
    _assert_pad_untouched(wbuf, K * Di, 7.0)
    what = "wgrad %s K %d N %d slabs %d" % (tile, K, N, S)
    assert_within(Wacc, ref, bound(mag, N, S), what)
    assert_within(bacc, bref, bound(bmag, N, 1), what + " bias")
    return S


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("name", sorted(WGRAD))
def test_weight_gradient_tiles_and_slabs(hip, pkg, cus256, name, K):
    """every tile of the weight gradient, accumulating onto non-zero W and bias.  200 rows: one slab (a slab has at least 256 rows).
    4 001 rows: these shapes have at most 6 tiles, so two rounds of even one block per CU (512 slots) ask for 85 slabs or more and the
    256-row minimum decides: ceil(4 001 / 256) = 16 slabs of ceil(4 001 / 16) = 251 -> 256 rows, the last one 161 rows, short and ragged.
    (With the minimum deciding, the count is the same without the rounding to 32 rows; the 64 x 64 case below pins the rounding.)"""
    Do, Di, tile = WGRAD[name]
    _wgrad_case(hip, pkg, Do, Di, K, 200, tile, slabs=1)
    _wgrad_case(hip, pkg, Do, Di, K, 4001, tile, slabs=16)


@pytest.mark.parametrize("K", [1, 3])
def test_weight_gradient_64x64_tiles(hip, pkg, cus256, K):
    """option wgrad_small: launches of at most that many rows on 64 x 64 tiles, two blocks per CU.  384 x 384: 36 tiles per tap;
    one tap: 512 / 36 = 14 slabs of ceil(3 700 / 14) = 265 -> 288 rows, which leaves 13 (the last one 244 rows); three taps: 108 tiles,
    4 slabs of 925 -> 928 rows.  One row more than the option's value: the 128 x 128 tile"""
    with options(pkg, wgrad_small=3700):
        _wgrad_case(hip, pkg, 384, 384, K, 3700, "64x64", slabs=13 if K == 1 else 4)
        _wgrad_case(hip, pkg, 384, 384, K, 200, "64x64", slabs=1)
    with options(pkg, wgrad_small=3699):
        _wgrad_case(hip, pkg, 384, 384, K, 3700, "128x128")
