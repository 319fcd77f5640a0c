"""CPU, one rank, no GPU: the ORDER of the argument checks of the entry points
that share a body with a sibling (plain / request-based one-sided calls, the
flushes, blocking / non-blocking reduction collectives, the any / some
completion calls, the tree hooks, the two op constructors).

Every case makes two or more arguments invalid at once; the error class that
comes back names the check that ran first.  Both forms of a pair are driven
from one case table.  No call here gets past its argument checks with work to
do: MPI_PROC_NULL targets and zero counts are the legal ways through."""
import ctypes

import numpy as np
import pytest

import msx

C = msx.C
i, i64, vp, u32 = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint
ip = ctypes.POINTER(ctypes.c_int)

IN_PLACE = vp(-1)
BAD_WIN = 0xA0000000 | 77
BAD_COMM = 0x1234
BAD_DT = 0x1234
BAD_REQ = 0x12345678
UNSET = 0x7777                       # a request word no call has written yet
INT, FLOAT, NUL = C.MPI_INT, C.MPI_FLOAT, C.MPI_DATATYPE_NULL
PN = C.MPI_PROC_NULL
E = C


def _fn(L, name, argtypes):
    """A function object of this module's own (CDLL[...] makes a fresh one), so
    the argument types set here do not leak into other test modules."""
    f = L[name]
    f.restype = i
    f.argtypes = argtypes
    return f


@pytest.fixture(scope="module")
def L():
    return msx.init(errors_return=True)


@pytest.fixture(scope="module")
def env(L):
    """One window (MPI_ERRORS_RETURN), a host user op, a device tree op, buffers."""
    buf = np.zeros(64, np.int32)
    a = np.zeros(64, np.int32)
    b = np.zeros(64, np.int32)
    win = i()
    assert L.MPI_Win_create(buf.ctypes.data, 256, 4, C.MPI_INFO_NULL, C.MPI_COMM_WORLD, ctypes.byref(win)) == 0
    assert L.MPI_Win_set_errhandler(win.value, C.MPI_ERRORS_RETURN) == 0
    UF = ctypes.CFUNCTYPE(None, vp, vp, ip, ip)
    fn = UF(lambda x, y, n, d: None)
    uop = i()
    assert L.MPI_Op_create(fn, 1, ctypes.byref(uop)) == 0
    DF = ctypes.CFUNCTYPE(i, vp, vp, i64, i, vp, vp)
    dfn = DF(lambda *_: 0)          # never entered: no call here reaches a launch
    top = i()
    assert L.msx_op_create_device_tree(dfn, dfn, 1, None, ctypes.byref(top)) == 0
    ns = dict(W=win.value, a=a.ctypes.data, b=b.ctypes.data, uop=uop.value, top=top.value,
              keep=(buf, a, b, fn, dfn))
    yield ns
    assert L.MPI_Op_free(ctypes.byref(uop)) == 0
    assert L.MPI_Op_free(ctypes.byref(top)) == 0
    assert L.MPI_Win_free(ctypes.byref(win)) == 0


def _sub(env, v):
    """Case tables are built at import time: names stand for the fixture's values."""
    return env[v[1:]] if isinstance(v, str) and v.startswith("$") else v


def _args(env, names, base, over):
    d = dict(base)
    d.update(over)
    assert set(over) <= set(names), over
    return [_sub(env, d[n]) for n in names]


def _wait(L, req):
    st = (i * 8)()
    assert L.MPI_Wait(ctypes.byref(req), st) == 0 and req.value == C.MPI_REQUEST_NULL


# ===========================================================================
# one-sided data movement: plain and request-based forms
# ===========================================================================
PG_NAMES = ["oaddr", "ocount", "odt", "rank", "disp", "tcount", "tdt", "win"]
PG_BASE = dict(oaddr="$a", ocount=8, odt=INT, rank=PN, disp=0, tcount=8, tdt=INT, win="$W")
PG_TYPES = [vp, i, i, i, i64, i, i, i]
PG_CASES = [
    ("proc_null", {}, 0),
    ("zero_count", dict(ocount=0, tcount=0, rank=0), 0),
    ("win>count", dict(win=BAD_WIN, ocount=-1), E.MPI_ERR_WIN),
    ("nullwin>type", dict(win=C.MPI_WIN_NULL, odt=NUL), E.MPI_ERR_WIN),
    ("ocount>otype", dict(ocount=-1, odt=NUL), E.MPI_ERR_COUNT),
    ("ocount>disp", dict(ocount=-1, disp=-1), E.MPI_ERR_COUNT),
    ("otype>rank", dict(odt=NUL, rank=5), E.MPI_ERR_TYPE),
    ("otype>tcount", dict(odt=BAD_DT, tcount=-1), E.MPI_ERR_TYPE),
    ("obuf>tcount", dict(oaddr=None, tcount=-1), E.MPI_ERR_BUFFER),
    ("tcount>disp", dict(tcount=-1, disp=-1), E.MPI_ERR_COUNT),
    ("ttype>disp", dict(tdt=NUL, disp=-1), E.MPI_ERR_TYPE),
    ("disp>rank", dict(disp=-1, rank=5), E.MPI_ERR_DISP),
    ("rank>match", dict(rank=5, tdt=FLOAT), E.MPI_ERR_RANK),
    ("negrank>match", dict(rank=-7, tcount=4), E.MPI_ERR_RANK),
    ("match_type>match_count", dict(rank=0, tdt=FLOAT, tcount=4), E.MPI_ERR_TYPE),
    ("match_count", dict(rank=0, tcount=4), E.MPI_ERR_COUNT),
]

ACC_NAMES = PG_NAMES[:-1] + ["op", "win"]
ACC_BASE = dict(PG_BASE, op=C.MPI_SUM)
ACC_TYPES = PG_TYPES[:-1] + [i, i]
ACC_CASES = [
    ("proc_null", {}, 0),
    ("replace_proc_null", dict(op=C.MPI_REPLACE), 0),
    ("win>op", dict(win=BAD_WIN, op=C.MPI_OP_NULL), E.MPI_ERR_WIN),
    ("ocount>op", dict(ocount=-1, op=C.MPI_OP_NULL), E.MPI_ERR_COUNT),
    ("obuf>op", dict(oaddr=None, op=C.MPI_NO_OP), E.MPI_ERR_BUFFER),
    ("noop>disp", dict(op=C.MPI_NO_OP, disp=-1), E.MPI_ERR_OP),
    ("ophandle>tcount", dict(op=C.MPI_OP_NULL, tcount=-1), E.MPI_ERR_OP),
    ("sumwide>rank", dict(op=C.MSX_SUM_WIDE, rank=5), E.MPI_ERR_OP),
    ("userop>disp", dict(op="$uop", disp=-1), E.MPI_ERR_OP),
    ("tcount>rank", dict(tcount=-1, rank=5), E.MPI_ERR_COUNT),
    ("disp>rank", dict(disp=-1, rank=5), E.MPI_ERR_DISP),
    ("rank>match", dict(rank=5, tdt=FLOAT), E.MPI_ERR_RANK),
    ("match_type>match_count", dict(rank=0, tdt=FLOAT, tcount=4), E.MPI_ERR_TYPE),
    ("match_count", dict(rank=0, tcount=4), E.MPI_ERR_COUNT),
]

GACC_NAMES = ["oaddr", "ocount", "odt", "raddr", "rcount", "rdt", "rank", "disp", "tcount", "tdt", "op", "win"]
GACC_BASE = dict(ACC_BASE, raddr="$b", rcount=8, rdt=INT)
GACC_TYPES = [vp, i, i, vp, i, i, i, i64, i, i, i, i]
GACC_CASES = [
    ("proc_null", {}, 0),
    ("win>op", dict(win=BAD_WIN, op=C.MPI_OP_NULL), E.MPI_ERR_WIN),
    ("ophandle>ocount", dict(op=C.MPI_OP_NULL, ocount=-1), E.MPI_ERR_OP),
    ("noop_ignores_origin", dict(op=C.MPI_NO_OP, ocount=-1, odt=NUL), 0),
    ("ocount>rtype", dict(ocount=-1, rdt=NUL), E.MPI_ERR_COUNT),
    ("otype>rcount", dict(odt=NUL, rcount=-1), E.MPI_ERR_TYPE),
    ("rcount>disp", dict(rcount=-1, disp=-1), E.MPI_ERR_COUNT),
    ("rbuf>tcount", dict(raddr=None, tcount=-1), E.MPI_ERR_BUFFER),
    ("tcount>userop", dict(tcount=-1, op="$uop"), E.MPI_ERR_COUNT),
    ("disp>userop", dict(disp=-1, op="$uop"), E.MPI_ERR_DISP),
    ("rank>sumwide", dict(rank=5, op=C.MSX_SUM_WIDE), E.MPI_ERR_RANK),
    ("userop", dict(op="$uop"), E.MPI_ERR_OP),
    ("sumwide>match", dict(op=C.MSX_SUM_WIDE, rank=0, tcount=4), E.MPI_ERR_OP),
    ("result_match>origin_match", dict(rank=0, rdt=FLOAT, ocount=4), E.MPI_ERR_TYPE),
    ("origin_match", dict(rank=0, ocount=4), E.MPI_ERR_COUNT),
]

RMA = {
    "put": ("MPI_Put", "MPI_Rput", PG_NAMES, PG_BASE, PG_TYPES),
    "get": ("MPI_Get", "MPI_Rget", PG_NAMES, PG_BASE, PG_TYPES),
    "acc": ("MPI_Accumulate", "MPI_Raccumulate", ACC_NAMES, ACC_BASE, ACC_TYPES),
    "gacc": ("MPI_Get_accumulate", "MPI_Rget_accumulate", GACC_NAMES, GACC_BASE, GACC_TYPES),
}
RMA_PARAMS = [pytest.param(k, over, want, id=f"{k}-{cid}")
              for k, cases in (("put", PG_CASES), ("get", PG_CASES), ("acc", ACC_CASES), ("gacc", GACC_CASES))
              for cid, over, want in cases]


@pytest.mark.parametrize("kind,over,want", RMA_PARAMS)
def test_rma_check_order(L, env, kind, over, want):
    """Both forms inside one MPI_Win_lock_all epoch (the request forms need a
    passive-target epoch for a real target rank)."""
    plain, rform, names, base, types = RMA[kind]
    args = _args(env, names, base, over)
    assert L.MPI_Win_lock_all(0, env["W"]) == 0
    try:
        assert _fn(L, plain, types)(*args) == want, msx.last_error()
        req = i(UNSET)
        assert _fn(L, rform, types + [ip])(*args, ctypes.byref(req)) == want, msx.last_error()
        if want == 0:
            assert req.value not in (UNSET, C.MPI_REQUEST_NULL)     # a complete request
            _wait(L, req)
        elif want == E.MPI_ERR_WIN:
            assert req.value == UNSET                               # nothing is touched before the window check
        else:
            assert req.value == C.MPI_REQUEST_NULL
    finally:
        assert L.MPI_Win_unlock_all(env["W"]) == 0


@pytest.mark.parametrize("kind", list(RMA))
def test_rma_request_checks_come_right_after_the_window(L, env, kind):
    """rma_request_pre: the null request, then the epoch of the target, before
    any datatype, op or target check; the window check before both."""
    _, rform, names, base, types = RMA[kind]
    f = _fn(L, rform, types + [ip])
    call = lambda req, **over: f(*_args(env, names, base, over), req)
    req = i(UNSET)
    r = ctypes.byref(req)
    assert call(None, win=BAD_WIN) == E.MPI_ERR_WIN
    assert call(None, ocount=-1) == E.MPI_ERR_ARG
    assert call(None, rank=0, odt=NUL) == E.MPI_ERR_ARG              # null request before the epoch check
    assert call(None, disp=-1, rank=5) == E.MPI_ERR_ARG
    # rank 0 outside any passive epoch: MPI_ERR_RMA_SYNC before every later check
    over = dict(rank=0, ocount=-1, disp=-1)
    if "op" in names:
        over["op"] = C.MPI_OP_NULL
    assert call(r, **over) == E.MPI_ERR_RMA_SYNC and req.value == C.MPI_REQUEST_NULL
    # a rank outside the window's group is not an epoch error: v_target reports it
    req.value = UNSET
    assert call(r, rank=5) == E.MPI_ERR_RANK and req.value == C.MPI_REQUEST_NULL
    # MPI_Win_lock on the rank opens the epoch; the next failing check is the origin count
    assert L.MPI_Win_lock(C.MPI_LOCK_SHARED, 0, 0, env["W"]) == 0
    req.value = UNSET
    assert call(r, rank=0, ocount=-1, disp=-1) == E.MPI_ERR_COUNT and req.value == C.MPI_REQUEST_NULL
    assert L.MPI_Win_unlock(0, env["W"]) == 0


FLUSH_CASES = [
    ("win>rank", dict(win=BAD_WIN, rank=5), E.MPI_ERR_WIN),
    ("nullwin>rank", dict(win=C.MPI_WIN_NULL, rank=-7), E.MPI_ERR_WIN),
    ("rank", dict(rank=5), E.MPI_ERR_RANK),
    ("negrank", dict(rank=-7), E.MPI_ERR_RANK),
    ("proc_null", dict(rank=PN), 0),
    ("self", dict(rank=0), 0),
]


@pytest.mark.parametrize("over,want", [pytest.param(o, w, id=c) for c, o, w in FLUSH_CASES])
def test_flush_check_order(L, env, over, want):
    args = _args(env, ["rank", "win"], dict(rank=0, win="$W"), over)
    for name in ("MPI_Win_flush", "MPI_Win_flush_local"):
        assert _fn(L, name, [i, i])(*args) == want, name
    # the _all forms take the window alone
    want_all = want if want in (0, E.MPI_ERR_WIN) else 0
    for name in ("MPI_Win_flush_all", "MPI_Win_flush_local_all"):
        assert _fn(L, name, [i])(args[1]) == want_all, name


# ===========================================================================
# reduction collectives: blocking and non-blocking forms
# ===========================================================================
OPN = C.MPI_OP_NULL
AR_NAMES = ["sbuf", "rbuf", "count", "dt", "op", "comm"]
AR_BASE = dict(sbuf="$a", rbuf="$b", count=8, dt=INT, op=C.MPI_SUM, comm=C.MPI_COMM_WORLD)
AR_TYPES = [vp, vp, i, i, i, i]
AR_CASES = [
    ("zero_count", dict(count=0), 0),
    ("comm>count", dict(comm=C.MPI_COMM_NULL, count=-1), E.MPI_ERR_COMM),
    ("badcomm>op", dict(comm=BAD_COMM, op=OPN), E.MPI_ERR_COMM),
    ("count>op", dict(count=-1, op=OPN), E.MPI_ERR_COUNT),
    ("count>type", dict(count=-1, dt=NUL), E.MPI_ERR_COUNT),
    ("type>op", dict(dt=NUL, op=OPN), E.MPI_ERR_TYPE),
    ("rbuf>op", dict(rbuf=None, op=OPN), E.MPI_ERR_BUFFER),
    ("op>sbuf", dict(op=OPN, sbuf=None), E.MPI_ERR_OP),
    ("replace>inplace", dict(op=C.MPI_REPLACE, rbuf=IN_PLACE), E.MPI_ERR_OP),
    ("op_dtype>alias", dict(op=C.MPI_BAND, dt=FLOAT, sbuf="$b"), E.MPI_ERR_OP),
    ("zero_count_checks_op", dict(count=0, op=OPN, rbuf=IN_PLACE), E.MPI_ERR_OP),
    ("rbuf_inplace", dict(rbuf=IN_PLACE, sbuf=None), E.MPI_ERR_BUFFER),
    ("alias", dict(sbuf="$b"), E.MPI_ERR_BUFFER),
]

RD_NAMES = ["sbuf", "rbuf", "count", "dt", "op", "root", "comm"]
RD_BASE = dict(AR_BASE, root=0)
RD_TYPES = [vp, vp, i, i, i, i, i]
RD_CASES = [
    ("zero_count", dict(count=0), 0),
    ("comm>root", dict(comm=C.MPI_COMM_NULL, root=7), E.MPI_ERR_COMM),
    ("root>count", dict(root=7, count=-1), E.MPI_ERR_ROOT),
    ("negroot>op", dict(root=-1, op=OPN), E.MPI_ERR_ROOT),
    ("count>op", dict(count=-1, op=OPN), E.MPI_ERR_COUNT),
    ("type>op", dict(dt=NUL, op=OPN), E.MPI_ERR_TYPE),
    ("sbuf>op", dict(sbuf=None, op=OPN), E.MPI_ERR_BUFFER),
    ("op>rbuf", dict(op=OPN, rbuf=IN_PLACE), E.MPI_ERR_OP),
    ("zero_count_checks_op", dict(count=0, op=OPN, rbuf=IN_PLACE), E.MPI_ERR_OP),
    ("rbuf_inplace", dict(rbuf=IN_PLACE), E.MPI_ERR_BUFFER),
    ("alias", dict(sbuf="$b"), E.MPI_ERR_BUFFER),
]

RS_NAMES = ["sbuf", "rbuf", "counts", "dt", "op", "comm"]
RS_BASE = dict(AR_BASE, counts=[8])
del RS_BASE["count"]
RS_CASES = [
    ("zero_count", dict(counts=[0]), 0),
    ("comm>counts", dict(comm=C.MPI_COMM_NULL, counts=None), E.MPI_ERR_COMM),
    ("nullcounts>op", dict(counts=None, op=OPN), E.MPI_ERR_ARG),
    ("count>type", dict(counts=[-1], dt=NUL), E.MPI_ERR_COUNT),
    ("type>op", dict(dt=NUL, op=OPN), E.MPI_ERR_TYPE),
    ("sbuf>op", dict(sbuf=None, op=OPN), E.MPI_ERR_BUFFER),
    ("op>rbuf", dict(op=OPN, rbuf=IN_PLACE), E.MPI_ERR_OP),
    ("zero_count_checks_op", dict(counts=[0], op=OPN), E.MPI_ERR_OP),
    ("rbuf_inplace", dict(rbuf=IN_PLACE), E.MPI_ERR_BUFFER),
    ("alias", dict(sbuf="$b"), E.MPI_ERR_BUFFER),
]

RSB_CASES = [
    ("zero_count", dict(count=0), 0),
    ("comm>count", dict(comm=C.MPI_COMM_NULL, count=-1), E.MPI_ERR_COMM),
    ("count>type", dict(count=-1, dt=NUL), E.MPI_ERR_COUNT),
    ("count>op", dict(count=-1, op=OPN), E.MPI_ERR_COUNT),
    ("type>op", dict(dt=NUL, op=OPN), E.MPI_ERR_TYPE),
    ("sbuf>op", dict(sbuf=None, op=OPN), E.MPI_ERR_BUFFER),
    ("op>rbuf", dict(op=OPN, rbuf=IN_PLACE), E.MPI_ERR_OP),
    ("zero_count_checks_op", dict(count=0, op=OPN), E.MPI_ERR_OP),
    ("rbuf_inplace", dict(rbuf=IN_PLACE), E.MPI_ERR_BUFFER),
    ("alias", dict(sbuf="$b"), E.MPI_ERR_BUFFER),
]

COLL = {
    "allreduce": ("MPI_Allreduce", "MPI_Iallreduce", AR_NAMES, AR_BASE, AR_TYPES),
    "reduce": ("MPI_Reduce", "MPI_Ireduce", RD_NAMES, RD_BASE, RD_TYPES),
    "reduce_scatter": ("MPI_Reduce_scatter", "MPI_Ireduce_scatter", RS_NAMES, RS_BASE, AR_TYPES[:2] + [vp] + AR_TYPES[3:]),
    "reduce_scatter_block": ("MPI_Reduce_scatter_block", "MPI_Ireduce_scatter_block", AR_NAMES, AR_BASE, AR_TYPES),
}
COLL_PARAMS = [pytest.param(k, over, want, id=f"{k}-{cid}")
               for k, cases in (("allreduce", AR_CASES), ("reduce", RD_CASES), ("reduce_scatter", RS_CASES),
                                ("reduce_scatter_block", RSB_CASES))
               for cid, over, want in cases]


def _coll_args(env, names, base, over):
    args = _args(env, names, base, over)
    if "counts" in names:
        k = names.index("counts")
        if args[k] is not None:
            args[k] = (i * len(args[k]))(*args[k])
    return args


@pytest.mark.parametrize("kind,over,want", COLL_PARAMS)
def test_reduction_collective_check_order(L, env, kind, over, want):
    blocking, nonblocking, names, base, types = COLL[kind]
    args = _coll_args(env, names, base, over)
    assert _fn(L, blocking, types)(*args) == want, msx.last_error()
    req = i(UNSET)
    assert _fn(L, nonblocking, types + [ip])(*args, ctypes.byref(req)) == want, msx.last_error()
    if want == 0:
        # a zero count still creates a request (MPI_Allreduce returns after validation)
        assert req.value not in (UNSET, C.MPI_REQUEST_NULL)
        _wait(L, req)
    elif want == E.MPI_ERR_COMM:
        assert req.value == UNSET                   # the communicator check comes before the request's
    else:
        assert req.value == C.MPI_REQUEST_NULL


@pytest.mark.parametrize("kind", list(COLL))
def test_nonblocking_request_check_comes_right_after_the_communicator(L, env, kind):
    _, nonblocking, names, base, types = COLL[kind]
    f = _fn(L, nonblocking, types + [ip])
    call = lambda req, **over: f(*_coll_args(env, names, base, over), req)
    assert call(None, comm=C.MPI_COMM_NULL) == E.MPI_ERR_COMM
    assert call(None, dt=NUL, op=OPN) == E.MPI_ERR_ARG
    if "count" in names:
        assert call(None, count=-1) == E.MPI_ERR_ARG
    else:
        assert call(None, counts=[-1]) == E.MPI_ERR_ARG
    if "root" in names:
        assert call(None, root=7) == E.MPI_ERR_ARG


# ===========================================================================
# multi-request completion: any / some
# ===========================================================================
RNULL = C.MPI_REQUEST_NULL
ANY_CASES = [
    # (id, count, requests, index?, status?, want)
    ("count>null", -1, None, True, True, E.MPI_ERR_COUNT),
    ("count>index", -1, [RNULL], False, True, E.MPI_ERR_COUNT),
    ("nullreqs>request", 2, None, True, True, E.MPI_ERR_ARG),
    ("nullindex>request", 2, [RNULL, BAD_REQ], False, True, E.MPI_ERR_ARG),
    ("nullstatus>request", 2, [RNULL, BAD_REQ], True, False, E.MPI_ERR_ARG),
    ("nullindex_count0", 0, None, False, True, E.MPI_ERR_ARG),
    ("request", 2, [RNULL, BAD_REQ], True, True, E.MPI_ERR_REQUEST),
    ("request_first", 2, [BAD_REQ, RNULL], True, True, E.MPI_ERR_REQUEST),
    ("all_inactive", 2, [RNULL, RNULL], True, True, 0),
    ("count0", 0, None, True, True, 0),
]


def _reqs(vals):
    return None if vals is None else (i * max(1, len(vals)))(*vals)


@pytest.mark.parametrize("count,reqs,has_index,has_status,want",
                         [pytest.param(*c[1:], id=c[0]) for c in ANY_CASES])
def test_testany_waitany_check_order(L, count, reqs, has_index, has_status, want):
    testany = _fn(L, "MPI_Testany", [i, vp, ip, ip, vp])
    waitany = _fn(L, "MPI_Waitany", [i, vp, ip, vp])
    for which in ("test", "wait"):
        arr = _reqs(reqs)
        index, flag, st = i(-5), i(-5), (i * 8)()
        pi = ctypes.byref(index) if has_index else None
        ps = st if has_status else None
        rc = testany(count, arr, pi, ctypes.byref(flag), ps) if which == "test" else waitany(count, arr, pi, ps)
        assert rc == want, (which, msx.last_error())
        if want == 0:
            assert index.value == C.MPI_UNDEFINED
            assert which == "wait" or flag.value == 1
        else:
            assert index.value == -5               # no output is written before the checks pass


def test_testany_null_flag_comes_before_the_requests(L):
    testany = _fn(L, "MPI_Testany", [i, vp, ip, ip, vp])
    index, st = i(-5), (i * 8)()
    assert testany(2, _reqs([RNULL, BAD_REQ]), ctypes.byref(index), None, st) == E.MPI_ERR_ARG
    assert testany(-1, None, ctypes.byref(index), None, st) == E.MPI_ERR_COUNT


SOME_CASES = [
    # (id, incount, requests, outcount?, indices?, statuses?, want)
    ("count>null", -1, None, False, False, False, E.MPI_ERR_COUNT),
    ("nullreqs>request", 2, None, True, True, True, E.MPI_ERR_ARG),
    ("nulloutcount>request", 2, [RNULL, BAD_REQ], False, True, True, E.MPI_ERR_ARG),
    ("nullindices>request", 2, [RNULL, BAD_REQ], True, False, True, E.MPI_ERR_ARG),
    ("nullstatuses>request", 2, [RNULL, BAD_REQ], True, True, False, E.MPI_ERR_ARG),
    ("nulloutcount_count0", 0, None, False, True, True, E.MPI_ERR_ARG),
    ("request", 2, [RNULL, BAD_REQ], True, True, True, E.MPI_ERR_REQUEST),
    ("request_first", 2, [BAD_REQ, RNULL], True, True, True, E.MPI_ERR_REQUEST),
    ("all_inactive", 2, [RNULL, RNULL], True, True, True, 0),
    ("count0", 0, None, True, False, False, 0),
]


@pytest.mark.parametrize("incount,reqs,has_out,has_idx,has_st,want",
                         [pytest.param(*c[1:], id=c[0]) for c in SOME_CASES])
def test_testsome_waitsome_check_order(L, incount, reqs, has_out, has_idx, has_st, want):
    for name in ("MPI_Testsome", "MPI_Waitsome"):
        f = _fn(L, name, [i, vp, ip, vp, vp])
        out, idx, st = i(-5), (i * 4)(), (i * 16)()
        rc = f(incount, _reqs(reqs), ctypes.byref(out) if has_out else None, idx if has_idx else None,
               st if has_st else None)
        assert rc == want, (name, msx.last_error())
        if want == 0:
            assert out.value == C.MPI_UNDEFINED
        elif want == E.MPI_ERR_REQUEST:
            assert out.value == 0                  # *outcount = 0 before the requests are looked at
        else:
            assert out.value == -5


def test_any_some_complete_a_finished_request(L, env):
    """A zero-count MPI_Iallreduce on one rank is a request that is complete at
    once: each of the four calls finds it behind a null entry."""
    iallreduce = _fn(L, "MPI_Iallreduce", AR_TYPES + [ip])

    def live():
        arr = (i * 2)(RNULL, UNSET)
        req = ctypes.cast(ctypes.byref(arr, ctypes.sizeof(i)), ip)
        assert iallreduce(env["a"], env["b"], 0, INT, C.MPI_SUM, C.MPI_COMM_WORLD, req) == 0
        assert arr[1] not in (UNSET, RNULL)
        return arr

    index, flag, st = i(-5), i(-5), (i * 16)()
    arr = live()
    assert _fn(L, "MPI_Testany", [i, vp, ip, ip, vp])(2, arr, ctypes.byref(index), ctypes.byref(flag), st) == 0
    assert (index.value, flag.value, arr[1]) == (1, 1, RNULL)
    arr = live()
    index.value = -5
    assert _fn(L, "MPI_Waitany", [i, vp, ip, vp])(2, arr, ctypes.byref(index), st) == 0
    assert (index.value, arr[1]) == (1, RNULL)
    for name in ("MPI_Testsome", "MPI_Waitsome"):
        arr = live()
        out, idx = i(-5), (i * 4)(-5, -5, -5, -5)
        assert _fn(L, name, [i, vp, ip, vp, vp])(2, arr, ctypes.byref(out), idx, st) == 0
        assert (out.value, idx[0], arr[1]) == (1, 1, RNULL)


# ===========================================================================
# tree hooks: msx_reduce_tree_spec_dev / _done_dev / _user_dev
# ===========================================================================
TREE_NAMES = ["srcs", "P", "pm", "nl", "chain", "out", "count", "dt", "op"]
TREE_BASE = dict(srcs="$srcs", P=4, pm=0, nl=0, chain=0, out="$a", count=0, dt=INT, op=None)
OP_, ARG_, CNT_ = E.MPI_ERR_OP, E.MPI_ERR_ARG, E.MPI_ERR_COUNT
TREE_CASES = [
    # (id, overrides, spec_dev, done_dev, user_dev); op None = MPI_SUM for the
    # builtin hooks and the device tree op for the user hook
    ("zero_count", {}, 0, 0, 0),
    ("zero_count>op", dict(op=C.MPI_REPLACE, srcs=None), 0, OP_, OP_),      # spec_dev alone returns first
    ("op>count", dict(op=OPN, count=-1), OP_, OP_, OP_),
    ("op_dtype>shape", dict(dt=C.MPI_BYTE, P=3, count=8), OP_, OP_, ARG_),  # a device op takes any datatype
    ("hostop>shape", dict(op="$uop", P=3, count=8), OP_, OP_, OP_),
    ("count>shape", dict(count=-1, P=3), CNT_, ARG_, ARG_),
    ("count", dict(count=-1), CNT_, ARG_, CNT_),
    ("shape>zero_count", dict(P=3), 0, ARG_, ARG_),
    ("shape", dict(P=3, count=8), ARG_, ARG_, ARG_),
    ("P_too_large", dict(P=32, count=8), ARG_, ARG_, ARG_),
    ("null_srcs", dict(srcs=None, count=8), ARG_, ARG_, ARG_),
    ("null_out", dict(out=None, count=8), ARG_, ARG_, ARG_),
    ("nleaves", dict(nl=5, count=8), ARG_, ARG_, ARG_),
    ("neg_nleaves", dict(nl=-1, count=8), ARG_, ARG_, ARG_),
    ("pairmask", dict(pm=0x10, count=8), ARG_, ARG_, ARG_),
    ("chain_P17", dict(chain=1, P=17, count=8), ARG_, ARG_, ARG_),
    # the user hook's stricter shape rule
    ("chain_P1", dict(chain=1, P=1), 0, 0, ARG_),
    ("chain_pairmask", dict(chain=1, P=4, pm=1), 0, 0, ARG_),
    ("chain_nleaves", dict(chain=1, P=4, nl=2), 0, 0, ARG_),
    ("pairmask_past_nleaves", dict(nl=2, pm=0x4), 0, 0, ARG_),
    ("pairmask_in_nleaves", dict(nl=2, pm=0x2), 0, 0, 0),
]


@pytest.mark.parametrize("over,spec,done,user", [pytest.param(*c[1:], id=c[0]) for c in TREE_CASES])
def test_tree_hook_check_order(L, env, over, spec, done, user):
    srcs = (vp * 32)(*([env["a"]] * 32))
    e = dict(env, srcs=srcs)
    spec_dev = _fn(L, "msx_reduce_tree_spec_dev", [vp, i, u32, i, i, vp, i64, i, i, vp])
    done_dev = _fn(L, "msx_reduce_tree_done_dev",
                   [vp, i, u32, i, i, vp, vp, i, vp, i, vp, i, ctypes.c_uint64, i64, i, i, vp])
    user_dev = _fn(L, "msx_reduce_tree_user_dev", [vp, i, u32, i, i, i, vp, i64, i, i, vp])
    a = dict(zip(TREE_NAMES, _args(e, TREE_NAMES, TREE_BASE, over)))
    bop = C.MPI_SUM if a["op"] is None else a["op"]
    uop = env["top"] if a["op"] is None else a["op"]
    head = (a["srcs"], a["P"], a["pm"], a["nl"], a["chain"])
    assert spec_dev(*head, a["out"], a["count"], a["dt"], bop, None) == spec, msx.last_error()
    assert done_dev(*head, a["out"], None, 0, None, 1, None, 0, 5, a["count"], a["dt"], bop, None) == done, \
        msx.last_error()
    assert user_dev(*head, 0, a["out"], a["count"], a["dt"], uop, None) == user, msx.last_error()


def test_tree_hooks_own_later_checks(L, env):
    srcs = (vp * 32)(*([env["a"]] * 32))
    user_dev = _fn(L, "msx_reduce_tree_user_dev", [vp, i, u32, i, i, i, vp, i64, i, i, vp])
    done_dev = _fn(L, "msx_reduce_tree_done_dev",
                   [vp, i, u32, i, i, vp, vp, i, vp, i, vp, i, ctypes.c_uint64, i64, i, i, vp])
    # in_left belongs to the shape check: before the count
    assert user_dev(srcs, 4, 0, 0, 0, 2, env["a"], -1, INT, env["top"], None) == ARG_
    assert user_dev(srcs, 4, 0, 0, 0, 1, env["a"], -1, INT, env["top"], None) == CNT_
    # a builtin op has no tree function
    assert user_dev(srcs, 4, 0, 0, 0, 0, env["a"], 0, INT, C.MPI_SUM, None) == OP_
    # done_dev: the extra-destination and result-ready checks run before the zero-count return
    assert done_dev(srcs, 4, 0, 0, 0, env["a"], None, -1, None, 1, None, 0, 5, 0, INT, C.MPI_SUM, None) == ARG_
    assert done_dev(srcs, 4, 0, 0, 0, env["a"], None, 0, None, 1, None, 1, 5, 0, INT, C.MPI_SUM, None) == ARG_
    assert done_dev(srcs, 4, 0, 0, 0, env["a"], None, -1, None, 1, None, 0, 5, 0, INT, OPN, None) == OP_


# ===========================================================================
# the op pool: MPI_Op_create and msx_op_create_device(_tree)
# ===========================================================================
def test_op_constructors_check_order_and_share_one_pool(L, env):
    """Both null checks are MPI_ERR_ARG: the error text names the one that ran
    first.  The two constructors take the first free slot of one pool."""
    UF = ctypes.CFUNCTYPE(None, vp, vp, ip, ip)
    DF = ctypes.CFUNCTYPE(i, vp, vp, i64, i, vp, vp)
    fn, dfn = UF(lambda x, y, n, d: None), DF(lambda *_: 0)
    op_create = _fn(L, "MPI_Op_create", [vp, i, ip])
    dev_create = _fn(L, "msx_op_create_device", [vp, i, vp, ip])
    tree_create = _fn(L, "msx_op_create_device_tree", [vp, vp, i, vp, ip])
    op = i(UNSET)
    for call, first in ((lambda f, o: op_create(f, 1, o), "null user_fn"),
                        (lambda f, o: dev_create(f, 1, None, o), "null device function"),
                        (lambda f, o: tree_create(f, None, 1, None, o), "null device function")):
        good = fn if first == "null user_fn" else dfn
        assert call(None, None) == ARG_ and first in msx.last_error()
        assert call(None, ctypes.byref(op)) == ARG_ and first in msx.last_error() and op.value == UNSET
        assert call(good, None) == ARG_ and "null op" in msx.last_error()

    h1, h2, h3 = i(), i(), i()
    assert op_create(fn, 0, ctypes.byref(h1)) == 0
    assert dev_create(dfn, 1, None, ctypes.byref(h2)) == 0
    assert h1.value != h2.value and {h1.value & 0xFC000000, h2.value & 0xFC000000} == {0x98000000}
    com = i(-1)
    assert L.MPI_Op_commutative(h1.value, ctypes.byref(com)) == 0 and com.value == 0
    assert (L.msx_op_is_device(h1.value), L.msx_op_is_device(h2.value)) == (0, 1)
    first = h1.value
    # the freed slot is the next one handed out, whichever constructor asks
    assert L.MPI_Op_free(ctypes.byref(h1)) == 0 and h1.value == C.MPI_OP_NULL
    assert tree_create(dfn, dfn, 1, None, ctypes.byref(h3)) == 0 and h3.value == first
    assert (L.msx_op_is_device(h3.value), L.msx_op_has_device_tree(h3.value)) == (1, 1)
    assert L.MPI_Op_commutative(h3.value, ctypes.byref(com)) == 0 and com.value == 1
    assert L.MPI_Op_free(ctypes.byref(h3)) == 0
    assert op_create(fn, 1, ctypes.byref(h1)) == 0 and h1.value == first
    assert (L.msx_op_is_device(h1.value), L.msx_op_has_device_tree(h1.value)) == (0, 0)
    assert L.MPI_Op_free(ctypes.byref(h1)) == 0
    assert L.MPI_Op_free(ctypes.byref(h2)) == 0
