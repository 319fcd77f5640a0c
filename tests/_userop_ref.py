"""The four reference orders of the user-op collectives, in numpy: every one of
the p ranks is simulated step by step, each holding its own buffers, and a step
reads the partner's buffer as it stood BEFORE the step.  Written from the
comments above host_user_allreduce / _reduce / _reduce_scatter / _scan and the
reduce.cpp lines they cite -- not from the library's introspection, which the
tests of the combine plan compare against this.

g(a, b) is the user function: the new `inout` from in = a, inout = b.  The
reduce_scatter orders are simulated over whole vectors, which equals the
block-wise exchange for an element-wise g."""


def _pof2(p):
    v = 1
    while v * 2 <= p:
        v *= 2
    return v


def _fold(xs, g):
    """reduce.cpp:3858-3865: below 2 * rem the even rank sends to the odd rank
    above it, which computes Uop(tmp = even's, recvbuf = its own) and takes
    newrank rank // 2; the ranks from 2 * rem on take rank - rem.
    -> ({newrank: value}, real rank of each newrank)"""
    p = len(xs)
    rem = p - _pof2(p)
    v, real = {}, {}
    for r in range(p):
        if r < 2 * rem:
            if r % 2:
                v[r // 2], real[r // 2] = g(xs[r - 1], xs[r]), r
        else:
            v[r - rem], real[r - rem] = xs[r], r
    return v, real


def allreduce(xs, g, commutative):
    """Recursive doubling, reduce.cpp:3890-3925: at step mask the ranks
    newrank and newrank ^ mask exchange their values; a commutative op or a
    partner below combines Uop(tmp, recvbuf), else Uop(recvbuf, tmp) and tmp
    becomes the value.  A folded even rank gets its odd neighbour's result.
    -> the value of every rank"""
    p = len(xs)
    pof2 = _pof2(p)
    rem = p - pof2
    v, real = _fold(xs, g)
    mask = 1
    while mask < pof2:
        old = dict(v)
        for n in range(pof2):
            tmp = old[n ^ mask]
            v[n] = g(tmp, old[n]) if commutative or real[n ^ mask] < real[n] else g(old[n], tmp)
        mask *= 2
    return [v[r // 2] if r < 2 * rem else v[r - rem] for r in range(p)]


def reduce(xs, g, commutative, root):
    """The binomial tree, reduce.cpp:440-540: relative ranks from lroot = root
    (commutative) or 0; relrank k without bit `mask` receives from k | mask and
    combines Uop(tmp, recvbuf) (commutative) or Uop(recvbuf, tmp) with tmp
    becoming the value; a rank with the bit has sent and left.  -> root's value"""
    p = len(xs)
    lroot = root if commutative else 0
    v = [xs[(k + lroot) % p] for k in range(p)]          # by relative rank
    mask = 1
    while mask < p:
        for k in range(0, p, 2 * mask):
            if k | mask < p:
                tmp = v[k | mask]
                v[k] = g(tmp, v[k]) if commutative else g(v[k], tmp)
        mask *= 2
    return v[0]


def reduce_scatter(xs, g, commutative, pairwise):
    """-> every rank's value of the WHOLE vector; rank r keeps its block.
    Non-commutative: the recursive-doubling order of allreduce.  Commutative,
    below the long-message gate: the fold, then recursive halving with mask =
    pof2 / 2, ..., 1, each step Uop(tmp = partner's, mine) (reduce.cpp:
    917-1334); a folded even rank's block comes from its odd neighbour.  At or
    above the gate: pairwise, step i takes the block from rank - i,
    Uop(tmp, recvbuf)."""
    p = len(xs)
    if not commutative:
        return allreduce(xs, g, False)
    if pairwise:
        out = []
        for r in range(p):
            acc = xs[r]
            for i in range(1, p):
                acc = g(xs[(r - i) % p], acc)
            out.append(acc)
        return out
    pof2 = _pof2(p)
    rem = p - pof2
    v, _ = _fold(xs, g)
    mask = pof2 // 2
    while mask:
        old = dict(v)
        for n in range(pof2):
            v[n] = g(old[n ^ mask], old[n])
        mask //= 2
    return [v[r // 2] if r < 2 * rem else v[r - rem] for r in range(p)]


def scan(xs, g, commutative, exclusive):
    """IscanBuildTaskList reduce.cpp:5285-5576 / IexscanBuildTaskList
    :5671-5960: at step mask rank r exchanges its partial with r ^ mask (when
    that rank exists).  r above: Uop(tmp, partial) and Uop(tmp, recvbuf), the
    first such step of an exscan copying tmp to recvbuf; r below: Uop(tmp,
    partial) for a commutative op, else Uop(partial, tmp) with tmp becoming the
    partial.  -> every rank's recvbuf (None: left untouched)"""
    p = len(xs)
    part = list(xs)
    res = [None if exclusive else x for x in xs]
    mask = 1
    while mask < p:
        old = list(part)
        for r in range(p):
            dst = r ^ mask
            if dst >= p:
                continue
            tmp = old[dst]
            if r > dst:
                part[r] = g(tmp, old[r])
                res[r] = tmp if res[r] is None else g(tmp, res[r])
            else:
                part[r] = g(tmp, old[r]) if commutative else g(old[r], tmp)
        mask *= 2
    return res
