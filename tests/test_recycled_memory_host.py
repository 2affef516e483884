"""CPU-only: the inventory of tests/recycled_cases.py is complete.

Every entry point of include/ppca_hip.h whose first argument is a context, a dataset, a row-compressed handle or a communicator either
is driven by an inventory entry -- and so runs on dirtied memory in tests/test_gpu_recycled_memory.py -- or stands in EXEMPT with the
reason.  A pass added to the C-ABI later fails here until it joins the inventory.  Exemptions are for calls that enqueue no kernel and
take no scratch (accessors, *_free, create / destroy, the hooks themselves) and for the RCCL entry points, which need peers."""
import os
import re

import recycled_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLES = ("ppca_ctx", "ppca_dataset", "ppca_sparse", "ppca_comm")

EXEMPT = {
    # the context itself: no kernel, no scratch
    "ppca_ctx_destroy": "releases the context",
    "ppca_ctx_set_stream": "swaps the stream after a synchronisation; enqueues nothing",
    "ppca_ctx_synchronize": "waits for the stream",
    "ppca_ctx_trim": "returns the cached blocks to the device; every entry of Test A ends with it",
    "ppca_ctx_enable_timing": "sets a host flag",
    "ppca_ctx_kernel_time": "reads HIP events",
    # hooks: host integers of the context
    "ppca_ctx_set_grid_limit": "test hook: sets the workgroup cap, a host integer",
    "ppca_ctx_dirty_scratch": "the hook of these tests itself",
    # accessors and releases of the handles
    "ppca_dataset_free": "releases a handle",
    "ppca_dataset_len": "accessor",
    "ppca_dataset_output_size": "accessor",
    "ppca_sparse_free": "releases a handle",
    "ppca_sparse_len": "accessor",
    "ppca_sparse_output_size": "accessor",
    "ppca_sparse_nnz": "accessor",
    "ppca_sparse_build_seconds": "accessor",
    # RCCL: need peers (tests/test_gpu_parity.py and tests/test_gpu_priors.py run them over one and two ranks)
    "ppca_comm_create": "RCCL: needs peers",
    "ppca_comm_create_all": "RCCL: needs peers",
    "ppca_comm_destroy": "RCCL: needs peers",
    "ppca_comm_n_ranks": "accessor",
    "ppca_comm_rank": "accessor",
    "ppca_comm_allreduce": "RCCL: needs peers",
    "ppca_em_step_sharded": "RCCL: needs peers (its pass is ppca_em_accumulate + ppca_em_finalize, both in the inventory)",
    "ppca_em_step_group": "RCCL: needs peers",
    "ppca_mix_em_step_sharded": "RCCL: needs peers (its pass is ppca_mix_em_step's, in the inventory)",
}


def _declarations():
    """name -> the type of the first parameter, for every function include/ppca_hip.h declares."""
    text = open(os.path.join(ROOT, "include", "ppca_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(ppca_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        first = " ".join(m.group(2).split()).split(",")[0]
        out[m.group(1)] = first
    return out


def _in_scope():
    return sorted(n for n, first in _declarations().items() if any(re.search(r"\b%s\b" % h, first) for h in HANDLES))


def test_the_header_is_parsed_whole():
    from ppca_rs_amd import _lib

    assert set(_declarations()) == set(_lib.SIGNATURES)
    scope = _in_scope()
    assert len(scope) >= 100 and "ppca_em_step" in scope and "ppca_sparse_em_step" in scope and "ppca_em_step_group" in scope
    assert "ppca_em_finalize_host" not in scope and "ppca_model_download" not in scope


def test_every_pass_is_in_the_inventory_or_exempt():
    driven = set().union(*[e.symbols for e in RC.ENTRIES])
    scope = set(_in_scope())
    missing = sorted(scope - driven - set(EXEMPT))
    assert not missing, "C-ABI passes that no entry of tests/recycled_cases.py drives: %s" % missing
    assert not sorted(set(EXEMPT) & driven), "exempt and driven at once"
    assert not sorted(set(EXEMPT) - scope), "exemptions for symbols that are not there"
    assert not sorted(driven - set(_declarations())), "entries name symbols the header does not declare"
    assert all(reason.strip() for reason in EXEMPT.values())


def test_an_entry_names_the_symbols_its_source_calls():
    """Every ppca_* symbol an entry lists stands in the source of the inventory (a list cannot claim a pass nobody calls) or is reached
    through the Python API method of the same pass."""
    src = open(os.path.join(ROOT, "tests", "recycled_cases.py")).read() + open(os.path.join(ROOT, "ppca_rs_amd", "api.py")).read() \
        + open(os.path.join(ROOT, "ppca_rs_amd", "_lib.py")).read()
    for e in RC.ENTRIES:
        for s in e.symbols:
            assert re.search(r"\.%s\b" % s, src), (e.name, s)


def test_shapes_reach_the_engines_their_names_claim(hiplib):
    """ppca_path_kind and the size gates of the split pipeline (RC.engine_of; tests/state_size_cases.py's table) put every entry that
    names an engine on it; the GPU test asserts the same from the pipeline's own record of the run."""
    seen = set()
    for e in RC.ENTRIES:
        if e.engine is None:
            continue
        d, k = e.shape
        assert RC.engine_of(d, k, hiplib.ppca_path_kind(d, k)) == e.engine, e.name
        seen.add(e.engine)
    assert seen == {"em9", "em16", "lane", "solve4", "mfma"}
    assert set(RC.SPARSE_KS) == {3, 16} and RC.TILING["block_rows"] < RC.S.SPARSE[0] and RC.TILING["segment"] < RC.S.SPARSE[1]


def test_polluters_and_exemptions():
    names = [e.name for e in RC.ENTRIES]
    assert len(names) == len(set(names))
    assert len(RC.POLLUTERS) == 5 and set(RC.POLLUTERS) <= set(names)
    assert RC.BIT_EXEMPT == {}  # (an entry compared by tolerance cites the line that makes its bits depend on more than its inputs)
