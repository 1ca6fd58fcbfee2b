#!/usr/bin/env python3
"""Development aid (round 8): searches the POST-PHASE of a 64-slot selection network for what the float32 fast path reads
(clip_fast32: ranks 0..4, 29..34 and 59..63 in order on their wires; everything else is only summed).

Pre-phase: the column is an R x C matrix in wire order (wire = C * row + column); the rows are sorted, then the columns
(rows stay sorted).  A 0-1 input is then a staircase matrix - C(R + C, R) of them (8 x 8: 12 870, 4 x 16: 4 845) - so any
post-phase is verified EXHAUSTIVELY, by the 0-1 principle, in well under a millisecond: every wire is one Python integer
with one bit per staircase case, and a sorter is a handful of AND / OR on them.

What the post-phase has to deliver (all four are checked on every case, `violations`):
  needed wires   wires 0..4, 29..34, 59..63 carry exactly those ranks;
  ends           (part of the above) wire 0 the minimum, wire 63 the maximum;
  sides          every value on wires 4..28 <= every value on wires 35..59;
  standard form  every sorter lists its wires ascending, minimum to the lowest (by construction of the moves).

Cost = instructions as stack_sort.h prices them: 2-sorter 2, 3-sorter 3, 4-sorter 7.

Search: start from Batcher's 64-network on those wires, drop what never swaps on the staircase cases, remove sorters greedily
while the properties hold; then local search with random restarts: fuse two sorters that share wires into one 3-sorter, widen
a 2-sorter by a wire, move a sorter's wire, each followed by greedy removal; a move is kept when the cost does not rise.

  search_select_grid.py [--grid R C] [--seed S] [--seconds T] [--no-sides] [--start FILE]
Prints the best post-phase as a table in the form of kSort16Ops / kMerge16Ops.
"""
import argparse
import random
import time

NP, T = 64, 4
# (ranks T and NP - T - 1 as well: the clip tests the first value BEHIND a full tail - would a fifth one go? - trim_low_fast / trim_high_fast)
NEED = list(range(T + 1)) + list(range((NP - T - 1) // 2, (NP + T) // 2 + 1)) + list(range(NP - T - 1, NP))
LOW = list(range(T, (NP - T - 1) // 2))                  # core below the median window
HIGH = list(range((NP + T) // 2 + 1, NP - T))            # core above it
PRICE = {2: 2, 3: 3, 4: 7}


def staircases(R, C):
    """Zeros per row, non-increasing down the rows (rows and columns sorted ascending, zeros first)."""
    out = []

    def rec(r, prev, acc):
        if r == R:
            out.append(tuple(acc))
            return
        for z in range(prev, -1, -1):
            rec(r + 1, z, acc + [z])

    rec(0, C, [])
    return out


def batcher(P2, p0=1):
    ces = []
    p = p0
    while p < P2:
        k = p
        while k >= 1:
            j = k % p
            while j <= P2 - 1 - k:
                lim = min(k - 1, P2 - j - k - 1)
                for i in range(lim + 1):
                    if (i + j) // (p * 2) == (i + j + k) // (p * 2):
                        ces.append((i + j, i + j + k))
                j += 2 * k
            k //= 2
        p *= 2
    return ces


class Problem:
    def __init__(self, R, C, sides=True):
        cases = staircases(R, C)
        self.ncases = len(cases)
        self.init = [0] * NP
        zeros = []
        for n, zs in enumerate(cases):
            zeros.append(sum(zs))
            for r in range(R):
                for c in range(zs[r], C):
                    self.init[r * C + c] |= 1 << n
        self.full = (1 << self.ncases) - 1
        self.expect = {}
        for w in NEED:
            e = 0
            for n, z in enumerate(zeros):
                if w >= z:
                    e |= 1 << n
            self.expect[w] = e
        self.low_zero = 0       # cases in which the low core must be all zeros
        self.high_one = 0       # cases in which the high core must be all ones
        for n, z in enumerate(zeros):
            if z >= LOW[-1] + 1:
                self.low_zero |= 1 << n
            if z <= HIGH[0]:
                self.high_one |= 1 << n
        self.sides = sides

    @staticmethod
    def apply(v, op):
        k = len(op)
        if k == 2:
            a, b = v[op[0]], v[op[1]]
            v[op[0]], v[op[1]] = a & b, a | b
        elif k == 3:
            a, b, c = v[op[0]], v[op[1]], v[op[2]]
            ab = a & b
            v[op[0]], v[op[1]], v[op[2]] = ab & c, ab | ((a | b) & c), a | b | c
        else:
            a, b, c, d = (v[w] for w in op)
            ab, cd, aob, cod = a & b, c & d, a | b, c | d
            v[op[0]] = ab & cd
            v[op[1]] = (ab & cod) | (cd & aob)                # at least three ones
            v[op[2]] = ab | cd | (aob & cod)                  # at least two
            v[op[3]] = aob | cod

    def ok(self, v):
        for w in NEED:
            if v[w] != self.expect[w]:
                return False
        if self.sides:
            for w in LOW:
                if v[w] & self.low_zero:
                    return False
            for w in HIGH:
                if (v[w] & self.high_one) != self.high_one:
                    return False
        return True

    def run(self, ops, v=None):
        v = list(self.init) if v is None else list(v)
        for op in ops:
            self.apply(v, op)
        return v

    def valid(self, ops):
        return self.ok(self.run(ops))


def cost(ops):
    return sum(PRICE[len(o)] for o in ops)


def drop_idle(P, ops):
    """Removes every sorter that changes nothing on any case."""
    v = list(P.init)
    keep = []
    for op in ops:
        before = [v[w] for w in op]
        P.apply(v, op)
        if before != [v[w] for w in op]:
            keep.append(op)
    return keep


def shrink(P, ops, rng, narrow=True):
    """Greedy removal (and narrowing of 3-/4-sorters by a wire) in random order while the network stays valid."""
    ops = list(ops)
    changed = True
    while changed:
        changed = False
        # prefix states, so that a trial re-runs only the tail
        pre = [list(P.init)]
        for op in ops:
            v = list(pre[-1])
            P.apply(v, op)
            pre.append(v)
        order = list(range(len(ops)))
        rng.shuffle(order)
        dead = set()
        first = len(ops)                    # the prefix states are those of the current network below this index only
        for i in order:
            start = min(i, first)
            trials = [None]
            if narrow and len(ops[i]) > 2:
                trials += [tuple(w for w in ops[i] if w != x) for x in ops[i]]
            for t in trials:
                tail = []
                for j in range(start, len(ops)):
                    if j in dead:
                        continue
                    if j == i:
                        if t is not None:
                            tail.append(t)
                    else:
                        tail.append(ops[j])
                if P.ok(P.run(tail, pre[start])):
                    if t is None:
                        dead.add(i)
                    else:
                        ops[i] = t
                    first = start
                    changed = True
                    break
        ops = [o for j, o in enumerate(ops) if j not in dead]
        ops = drop_idle(P, ops)
    return ops


def mutate(P, ops, rng):
    ops = list(ops)
    n = len(ops)
    kind = rng.random()
    i = rng.randrange(n)
    if kind < 0.45:
        # fuse op i with a later op that shares a wire, union of at most 3 wires (4 seldom pays: 7 instructions)
        cand = [j for j in range(i + 1, min(n, i + 40)) if set(ops[i]) & set(ops[j]) and len(set(ops[i]) | set(ops[j])) <= 3]
        if not cand:
            return None
        j = rng.choice(cand)
        u = tuple(sorted(set(ops[i]) | set(ops[j])))
        if rng.random() < 0.5:
            ops[j] = u
            del ops[i]
        else:
            ops[i] = u
            del ops[j]
    elif kind < 0.75:
        # widen a 2-sorter by one wire
        if len(ops[i]) != 2:
            return None
        w = rng.randrange(NP)
        if w in ops[i]:
            return None
        ops[i] = tuple(sorted(ops[i] + (w,)))
    elif kind < 0.9:
        # move one wire of a sorter
        w = rng.randrange(NP)
        if w in ops[i]:
            return None
        o = list(ops[i])
        o[rng.randrange(len(o))] = w
        ops[i] = tuple(sorted(o))
    else:
        # insert a fresh 3-sorter
        ws = rng.sample(range(NP), 3)
        ops.insert(i, tuple(sorted(ws)))
    return ops


def table(ops, name):
    rows = []
    for o in ops:
        w = list(o) + [0] * (4 - len(o))
        rows.append('{{%d, %d, %d, %d}, %d}' % (w[0], w[1], w[2], w[3], len(o)))
    lines = ['constexpr NetOp %s[%d] = {' % (name, len(ops))]
    for k in range(0, len(rows), 6):
        lines.append('    ' + ', '.join(rows[k:k + 6]) + (',' if k + 6 < len(rows) else '};'))
    return '\n'.join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grid', type=int, nargs=2, default=[8, 8])
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--seconds', type=float, default=60)
    ap.add_argument('--no-sides', action='store_true')
    ap.add_argument('--start', help='file with a python list of wire tuples to start from')
    a = ap.parse_args()
    R, C = a.grid
    rng = random.Random(a.seed)
    P = Problem(R, C, sides=not a.no_sides)
    pre_cost = {(8, 8): 16 * 24, (4, 16): 4 * 86 + 16 * 7}.get((R, C), 0)
    if a.start:
        cur = [tuple(o) for o in eval(open(a.start).read())]
        assert P.valid(cur)
    else:
        full = [tuple(o) for o in batcher(NP)]
        assert P.valid(full)
        cur = drop_idle(P, full)
        print('grid %d x %d: %d cases; Batcher %d -> never idle %d' % (R, C, P.ncases, len(full), len(cur)), flush=True)
        cur = shrink(P, cur, rng)
    print('greedy: %d sorters, %d instructions (+ pre-phase %d = %d)' % (len(cur), cost(cur), pre_cost, cost(cur) + pre_cost), flush=True)
    best = cur
    t0 = time.time()
    tried = kept = 0
    while time.time() - t0 < a.seconds:
        m = mutate(P, cur, rng)
        if m is None:
            continue
        tried += 1
        if not P.valid(m):
            continue
        m = shrink(P, m, rng)
        if cost(m) <= cost(cur):
            kept += 1
            if cost(m) < cost(best):
                best = m
                print('%6.0f s  %5d moves: %d sorters, %d instructions (total %d)' % (time.time() - t0, tried, len(m), cost(m), cost(m) + pre_cost), flush=True)
            cur = m
    assert P.valid(best)
    cnt = {k: sum(1 for o in best if len(o) == k) for k in (2, 3, 4)}
    print('best: %d instructions (%d 2-sorters, %d 3-sorters, %d 4-sorters), pre-phase %d, total %d; %d moves tried, %d kept'
          % (cost(best), cnt[2], cnt[3], cnt[4], pre_cost, cost(best) + pre_cost, tried, kept))
    print(best)
    print(table(best, 'kSelect%dx%dOps' % (R, C)))


if __name__ == '__main__':
    main()
