"""The account of what a handle holds between calls (Holds, clima_amd/csrc/radtran_dev.h) and the one refusal function
every entry point asks (refused), replayed through clima_test_handle_holds: no handle, no device.

A table of transition sequences with the outcome written out.  The rule behind the batch rows: after a batch the handle
holds what n single calls would have left -- but for the column (a resident call needs an upload first) and, where the
batch ran one launch per chunk, the optical properties (they stayed in the batch's own memory)."""
import ctypes as C

import pytest

EVENT_N, OUT_N = 6, 14      # CLIMA_HOLDS_EVENT_N, CLIMA_HOLDS_OUT_N (include/clima_radtran_hip.h)
OUT = ("column", "particles", "uploads", "opr", "w0_stored", "opr_upload", "opr_lo", "opr_n", "rows_on_host",
       "rows_in_pinned", "refuses_column", "refuses_opacities", "refuses_spectrum", "opr_of_resident")
NW = 8                      # opacity bins of the imagined handle


# ---- the transitions by name (the hook's codes)
def uploaded(particles=False):
    return (0, particles)


def opacities_written(own_block=True, w0_stored=True, from_resident=True, lo=0, n=NW):
    return (1, own_block, w0_stored, from_resident, lo, n)


W0_FORMED, ROWS_CHANGED, ROWS_FETCHED, BATCH_REPEATED, RESULTS_DROPPED = (2,), (4,), (5,), (7,), (8,)


def rows_enqueued(in_pinned=False):
    return (3, in_pinned)


def batch_left(one_launch, np=0):
    return (6, one_launch, np)


def single_call(w0_stored=True, in_pinned=True, lo=0, n=NW):
    """a synchronous radiate(): upload, opacity pass, integration, fetch"""
    return [uploaded(), opacities_written(True, w0_stored, True, lo, n), rows_enqueued(in_pinned), ROWS_FETCHED]


def column_call(lo=0, n=NW):
    """one column of a batch that runs one call per column: the handle's own block, not the resident column"""
    return [opacities_written(True, True, False, lo, n), rows_enqueued(False)]


CHUNK = [opacities_written(own_block=False), rows_enqueued(False)]      # one launch of a one-launch batch


def holds(L, events, shard_world=1, comm=False, op_lo=0, op_n=NW):
    flat = [shard_world, int(comm), op_lo, op_n]
    for e in events:
        flat += [int(v) for v in e] + [0] * (EVENT_N - len(e))
    out = (C.c_int * OUT_N)(*([-7] * OUT_N))
    L.clima_test_handle_holds(C.byref(C.c_int(len(events))), (C.c_int * len(flat))(*flat), out)
    return dict(zip(OUT, out))


FRESH = dict(column=0, particles=0, uploads=0, opr=0, w0_stored=1, opr_upload=0, opr_lo=0, opr_n=0, rows_on_host=0,
             rows_in_pinned=0, refuses_column=1, refuses_opacities=1, refuses_spectrum=0, opr_of_resident=1)
AFTER_CALL = dict(FRESH, column=1, uploads=1, opr=1, opr_upload=1, opr_n=NW, rows_on_host=1, rows_in_pinned=1,
                  refuses_column=0, refuses_opacities=0)

TABLE = [
    ("a fresh handle", [], FRESH),
    ("upload only", [uploaded(True)], dict(FRESH, column=1, particles=1, uploads=1, refuses_column=0, opr_of_resident=0)),
    ("an opacity call that stored w0", single_call(), AFTER_CALL),
    ("an opacity call that left w0 to the fused grid", single_call(w0_stored=False), dict(AFTER_CALL, w0_stored=0)),
    ("... and the IR-only call behind it formed w0", single_call(w0_stored=False) + [W0_FORMED, rows_enqueued(False)],
     dict(AFTER_CALL, rows_on_host=0, rows_in_pinned=0)),
    ("a second upload: the opacities are the first column's", single_call() + [uploaded()],
     dict(AFTER_CALL, uploads=2, opr_of_resident=0)),
    ("a one-launch batch: column gone, opacities refused", single_call() + CHUNK + CHUNK + [batch_left(True), ROWS_CHANGED],
     dict(AFTER_CALL, column=0, opr=0, rows_on_host=0, rows_in_pinned=0, refuses_column=1, refuses_opacities=1)),
    ("a one-launch batch on a fresh handle, particle columns", CHUNK + [batch_left(True, 2), ROWS_CHANGED],
     dict(FRESH, particles=1)),
    ("a batch of one call per column: opacities accepted, column gone",
     [column_call(), column_call(), [batch_left(False), ROWS_CHANGED]],
     dict(FRESH, opr=1, opr_n=NW, refuses_opacities=0)),
    ("a one-launch batch, then its repeat", CHUNK + [batch_left(True)] + column_call() + column_call() + [BATCH_REPEATED, ROWS_CHANGED],
     dict(FRESH, opr=1, opr_n=NW, refuses_opacities=0)),
    ("a graph replay: opacities refused, the column stays", single_call() + [rows_enqueued(False), RESULTS_DROPPED],
     dict(AFTER_CALL, opr=0, rows_on_host=0, rows_in_pinned=0, refuses_opacities=1)),
    ("rows changed behind the host's back", single_call() + [ROWS_CHANGED], dict(AFTER_CALL, rows_on_host=0, rows_in_pinned=0)),
    ("... and fetched again", single_call() + [ROWS_CHANGED, ROWS_FETCHED], dict(AFTER_CALL, rows_in_pinned=0)),
    ("a resident call: rows through the copy", single_call() + [rows_enqueued(False)],
     dict(AFTER_CALL, rows_on_host=0, rows_in_pinned=0)),
]
TABLE = [(name, [e for x in ev for e in (x if isinstance(x, list) else [x])], want) for name, ev, want in TABLE]


@pytest.mark.parametrize("name,events,want", TABLE, ids=[t[0] for t in TABLE])
def test_what_the_handle_holds(hip_lib, name, events, want):
    assert holds(hip_lib, events) == want


def test_opacities_cover_the_bins_asked_for(hip_lib):
    """written for bins [0, k) then asked for [k, m): refused; written for [0, m) then asked for [0, k): accepted"""
    k, m = 3, NW
    shard = single_call(lo=0, n=k)
    whole = single_call(lo=0, n=m)
    assert holds(hip_lib, shard, 2, False, 0, k)["refuses_opacities"] == 0          # the same shard
    assert holds(hip_lib, shard, 2, False, k, m - k)["refuses_opacities"] == 1       # the other shard
    assert holds(hip_lib, shard, 1, False, 0, m)["refuses_opacities"] == 1           # back to the whole spectrum
    assert holds(hip_lib, whole, 2, False, 0, k)["refuses_opacities"] == 0           # unsharded pass, then a shard
    assert holds(hip_lib, whole, 2, False, k, m - k)["refuses_opacities"] == 0
    assert holds(hip_lib, single_call(lo=k, n=m - k), 3, False, k + 1, 2)["refuses_opacities"] == 0   # a range inside
    assert holds(hip_lib, single_call(lo=k, n=m - k), 3, False, k - 1, 2)["refuses_opacities"] == 1   # ... straddling its start
    assert holds(hip_lib, single_call(lo=0, n=k), 3, False, k - 1, 2)["refuses_opacities"] == 1       # ... its end
    # valid is still required: the bins alone do not make opacities
    assert holds(hip_lib, whole + [RESULTS_DROPPED], 1, False, 0, m)["refuses_opacities"] == 1


@pytest.mark.parametrize("world,comm,spectrum", [(1, False, 0), (2, False, 1), (2, True, 0)])
@pytest.mark.parametrize("events,column,opacities", [([], 1, 1), ([uploaded()], 0, 1), (single_call(), 0, 0),
                                                     (single_call() + CHUNK + [batch_left(True)], 1, 1)],
                         ids=["fresh", "uploaded", "called", "one-launch batch"])
def test_every_need_on_every_shard(hip_lib, world, comm, spectrum, events, column, opacities):
    """the whole spectrum is refused on a shard without a communicator, whatever the handle holds; the column and the
    opacities by what it holds, whatever the shard (the stored block covers the bins asked for here)"""
    got = holds(hip_lib, events, world, comm, 0, NW)
    assert (got["refuses_column"], got["refuses_opacities"], got["refuses_spectrum"]) == (column, opacities, spectrum)


def test_an_unknown_transition_is_flagged(hip_lib):
    assert holds(hip_lib, [(99,)])["column"] == -1
