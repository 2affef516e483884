"""No pass depends on what its recycled device memory held.

Every output dataset and every scratch buffer of the library comes from the context's block cache or is kept by the context across
calls: in a training loop a pass never sees fresh memory.  The inventory of tests/recycled_cases.py runs here
  A  on one private context: twice as it comes, then after ppca_ctx_dirty_scratch(0xFF) (every double a NaN, every int -1: what a
     released masked dataset holds) and after (0x3F) (every double 4.8e-4, every int 1061109567) -- all four bit for bit equal;
  B  behind each of the five entries that leave the most behind (guard flags, a second-stage verdict, the split pipeline's workspace,
     a mixture's slice tables and row lists, the sparse passes' scratch) -- bit for bit what a context that ran nothing else gives;
  C  after the 0xFF fill against the oracle, at the tolerance of the existing test of the same quantity -- so that A and B cannot
     pass on an answer that is wrong the same way every time.
Bits are compared as bytes: NaN equals NaN, -0 differs from 0.
"""
import struct

import numpy as np
import pytest

import recycled_cases as RC

pytestmark = pytest.mark.gpu

FILLS = (0xFF, 0x3F)


@pytest.fixture(scope="module")
def P(hiplib):
    import ppca_rs_amd as p

    return p


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, (float, np.floating)):
        return isinstance(b, (float, np.floating)) and struct.pack("d", a) == struct.pack("d", b)
    return type(a) is type(b) and a == b


def _differing(got, want):
    """The keys on which two results differ, with the share of an array's elements that do."""
    if got.keys() != want.keys():
        return ["keys: %s" % sorted(set(got) ^ set(want))]
    out = []
    for key in want:
        if _same(got[key], want[key]):
            continue
        g, w = got[key], want[key]
        if isinstance(w, np.ndarray) and isinstance(g, np.ndarray) and g.shape == w.shape and g.dtype == w.dtype and w.dtype.itemsize in (4, 8):
            view = np.uint64 if w.dtype.itemsize == 8 else np.uint32
            bad = np.ascontiguousarray(g).view(view) != np.ascontiguousarray(w).view(view)
            first = np.argwhere(bad)[0]
            out.append("%s: %d of %d elements, first at %s: %r != %r" % (key, int(bad.sum()), bad.size, tuple(first), g[tuple(first)],
                                                                     w[tuple(first)]))
        else:
            out.append("%s: %r != %r" % (key, g, w))
    return out


def _assert_same(got, want, what):
    diff = _differing(got, want)
    assert not diff, (what, diff)


_R0, _R2 = {}, {}


def _context():
    from ppca_rs_amd import _lib

    return _lib.Context(0)


def _r0(P, entry):
    """The entry's result on a context that ran nothing else; computed once per entry and shared."""
    if entry.name not in _R0:
        ctx = _context()
        try:
            _R0[entry.name] = entry.run(P, ctx)
        finally:
            ctx.trim()
    return _R0[entry.name]


def _dirty(ctx, fill, entry):
    blocks, nbytes = ctx.dirty_scratch(fill)
    assert blocks >= 1 and nbytes >= entry.biggest, ("nothing of the entry's size was cached", entry.name, blocks, nbytes, entry.biggest)


def test_inventory_is_unique_and_has_no_exemption():
    names = [e.name for e in RC.ENTRIES]
    assert len(set(names)) == len(names) and set(RC.POLLUTERS) <= set(names)
    assert RC.BIT_EXEMPT == {}, "an entry that is not compared bit for bit cites the line that makes it so, in DESIGN.md 4.29 too"


@pytest.mark.parametrize("entry", RC.ENTRIES, ids=lambda e: e.name)
def test_dirty_scratch(P, entry):
    """A: R0, R1 as the context comes; R2 after the 0xFF fill; R3 after the 0x3F fill."""
    ctx = _context()
    try:
        r0 = entry.run(P, ctx)
        _R0.setdefault(entry.name, r0)
        r1 = entry.run(P, ctx)
        _dirty(ctx, FILLS[0], entry)
        r2 = entry.run(P, ctx)
        _R2.setdefault(entry.name, r2)
        _dirty(ctx, FILLS[1], entry)
        r3 = entry.run(P, ctx)
    finally:
        ctx.trim()
    _assert_same(r1, r0, "R1 != R0: the pass does not reproduce itself on one context")
    _assert_same(r2, r0, "R2 != R0: the pass read a byte of the 0xFF fill")
    _assert_same(r3, r0, "R3 != R0: the pass read a byte of the 0x3F fill")
    if entry.engine and entry.engine != "em9":  # the shape reached the engine its name claims (the split pipeline's own record)
        t = r0.get("trace_out") or r0.get("trace_em")
        if t is not None:
            assert t["valid"] == 1 and (t["d"], t["k"]) == entry.shape
            if "trace_em" in r0:
                assert r0["trace_em"]["fused16"] == (1 if entry.engine == "em16" else 0)
            if "trace_out" in r0:
                assert r0["trace_out"]["solver"] in RC.SOLVER_OF[entry.engine], r0["trace_out"]["solver"]


@pytest.mark.parametrize("entry", RC.ENTRIES, ids=lambda e: e.name)
@pytest.mark.parametrize("polluter", RC.POLLUTERS)
def test_after_a_polluter(P, polluter, entry):
    """B: the polluter, then the entry, on one private context."""
    want = _r0(P, entry)
    ctx = _context()
    try:
        RC.by_name(polluter).run(P, ctx)
        got = entry.run(P, ctx)
    finally:
        ctx.trim()
    _assert_same(got, want, "the pass depends on what %s left on the context" % polluter)


@pytest.mark.parametrize("entry", [e for e in RC.ENTRIES if e.oracle], ids=lambda e: e.name)
def test_dirtied_result_against_oracle(P, oracle, entry):
    """C: R2 against the oracle, at the tolerances of the existing comparison of the same entry (cited at its `oracle`)."""
    if entry.name not in _R2:
        ctx = _context()
        try:
            entry.run(P, ctx)
            _dirty(ctx, FILLS[0], entry)
            _R2[entry.name] = entry.run(P, ctx)
        finally:
            ctx.trim()
    entry.oracle(oracle, _R2[entry.name])


def test_the_variants_take_their_second_stages(P):
    """The guard-tripping model and the outlier row do reach what they are in the inventory for (otherwise they pollute nothing)."""
    assert _r0(P, RC.by_name("step_guard_256x10"))["guard"][0] == 1
    out = _r0(P, RC.by_name("step_outlier_256x10"))
    assert out["guard"] == (0, 1) and out["fallback"] == (2, 1, 32), (out["guard"], out["fallback"])  # one workgroup's slice of seven
    assert _r0(P, RC.by_name("step_outlier_200x16"))["counters"][7] >= 1  # (the two-kernel pass: its workgroups that went to fp64)
    assert _r0(P, RC.by_name("engine_em9_256x10"))["guard"] == (0, 0)
    assert _r0(P, RC.by_name("step_guard_200x16"))["gram_engine"] == 1 and _r0(P, RC.by_name("engine_em16_200x13"))["gram_engine"] == 0
