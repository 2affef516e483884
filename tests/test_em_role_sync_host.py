"""The hand-off protocol of the fused EM pass's front role (ppca_em9.hip), restated as a small model and
run under random schedules on the CPU.

Four front waves and the back role (one agent: its four waves move in lockstep on their own barrier) are step lists of the kinds
arrive (add to a monotonic counter), wait (until a counter reaches a target), read region, write region.  An access may name a
share (`part`): the four waves stage, or store [G | b] into, disjoint rows / columns of one region; two accesses conflict when
one of them is a write, they come from different agents and their shares overlap (no share = the whole region).

Ordering is what the counters give and nothing else: an arrive publishes the agent's vector clock into the counter, a wait that
succeeds joins the counter's clock into the agent's (a wave's LDS operations execute in order, so its add follows its earlier
reads and writes; a wave that has seen the count comes after every add that made it).  A schedule fails when it deadlocks or when
a region is written while an access of another agent that is not ordered in front of the write is still open, or read while such
a write is.

The ledger (the same as in the header comment of ppca_em9.hip).  T = tiles of the workgroup, trips rel = 0 .. T, trip T is the
extra trip (no tile: `cur` false); solver(rel) = rel mod 4; the back role makes iterations r = 0 .. T - 1.

    counter  who adds, how much, where                                       waiter: target
    fbar     every front wave 1 at: the prologue barrier; F1 (in front of     the same waves, 4 per barrier passed: prologue 4; F1 of
             phase beta) of trips 0 .. T; F3 (behind P4a) and F4 (behind      trip rel 4 (3 rel + 2); F3 4 (3 rel + 3); F4
             the staging) of trips < T; the epilogue barrier                  4 (3 rel + 4); epilogue 4 (3 T + 3)
    cbar     every column wave 1 behind its factor loads, trips 1 .. T        the column waves in front of their wP stores: 3 rel
    solved   solver(rel) 1 behind its last store, trips < T                   the other three, behind P4a's table and mean requests,
                                                                             in front of its first read of the tile's [wz | w]:
                                                                             rel + 1
    wready   every front wave 1 behind its OWN phase-beta stores, trips       back role, iteration r: 4 (r + 1)
             1 .. T
    digdone  back role 4 per tile behind its last read of the W rows          front, in front of its [G | b] stores of trip
                                                                             rel >= 2: 4 (rel - 1)
    itdone   back role 4 per tile at the end of its iteration                 front, in front of the staging of trip rel >= 2:
                                                                             4 (rel - 1)

The model also knows the two hand-offs that were measured and not kept (`variant="three"`: p2done, 4 per trip, waited for by the
solver alone in place of F1; xfree, 4 per trip behind P4a's last read of the x~ tile, waited for in front of the staging's first
x~ store in place of F3): they are as safe as what ships, they were not faster (profiles/em9_role_sync/README.md).
"""
import random

import pytest

NF = 4
BACK = 4  # agent index of the back role
NAG = 5


def closed_forms(T, variant="shipped"):
    """Every counter's value when a workgroup of T tiles has finished (the ledger's sums)."""
    if variant == "three":
        return {"fbar": 4 * (T + 2), "p2done": 4 * T, "cbar": 3 * T, "solved": T, "wready": 4 * T, "xfree": 4 * T,
                "digdone": 4 * T, "itdone": 4 * T}
    return {"fbar": 4 * (3 * T + 3), "cbar": 3 * T, "solved": T, "wready": 4 * T, "digdone": 4 * T, "itdone": 4 * T}


def front_steps(w, T, mutate=None, variant="shipped"):
    s = []
    three = variant == "three"
    passed = [0]  # barriers of the role this wave has passed

    def barrier():
        passed[0] += 1
        s.append(("arrive", "fbar", 1))
        s.append(("wait", "fbar", 4 * passed[0]))

    def arrive(c, k=1):
        s.append(("arrive", c, k))

    def wait(c, t):
        if t > 0:
            s.append(("wait", c, t))

    def read(r, part=None):
        s.append(("read", r, part))

    def write(r, part=None):
        s.append(("write", r, part))

    def stage(rel_next):  # the staging of tile rel_next: x~ rows, mask words, the per-dimension sample masks
        write("Xs", w)
        write("Ms%d" % (rel_next & 1), w)
        write("Mb%d" % (rel_next & 3), w)

    if T > 0:
        stage(0)  # prologue: nothing has read the x~ tile yet, no wait
    barrier()  # prologue
    for rel in range(T + 1):
        cur = rel < T
        par, prev, solver = rel & 1, (rel + 1) & 1, rel & 3
        if cur:  # P2: [G | b] of the tile
            read("Xs")
            read("Ms%d" % par)
            if rel >= 2:
                wait("digdone", 4 * (rel - 1))
            write("GA%d" % par, w)
            write("GB%d" % par, w)
            if three:
                arrive("p2done")
        if not three:
            barrier()  # F1
            assert mutate or 4 * passed[0] == 4 * (3 * rel + 2)
        # phase beta
        if w == solver:
            if cur:
                if three:
                    wait("p2done", 4 * (rel + 1))
                read("Ms%d" % par)
                read("GA%d" % par)
                read("GB%d" % par)
                write("GA%d" % par)  # factor (entry-major over the whole G part), z
                write("GB%d" % par)  # [wz | w]
                write("XT%d" % par)
                arrive("solved")
        elif rel > 0:
            cw = (w - solver - 1) & 3
            read("GA%d" % prev)  # factor and z of tile rel - 1
            read("Ms%d" % prev)
            arrive("cbar")
            wait("cbar", 3 * rel)
            write("GA%d" % prev, w)  # its columns of wP, where the factor was
            if cw == NF - 2:  # the tile's scalars
                read("XT%d" % prev)
                read("scl")
                write("scl")
        if rel > 0:
            arrive("wready")
        if not cur:
            break
        # P4a
        if w != solver and mutate != "no-solved-wait":
            wait("solved", rel + 1 + (1 if mutate == "solved-target" else 0))
        read("GB%d" % par)
        read("Xs")
        if three:
            arrive("xfree")
        elif mutate != "no-f3":
            barrier()  # F3: the x~ tile is free
            assert mutate or 4 * passed[0] == 4 * (3 * rel + 3)
        # staging of tile rel + 1
        if rel >= 2:
            wait("itdone", 4 * (rel - 1))
        if three and mutate != "no-xfree-wait":
            wait("xfree", 4 * (rel + 1))
        stage(rel + 1)
        barrier()  # F4
        assert three or mutate or 4 * passed[0] == 4 * (3 * rel + 4)
    barrier()  # epilogue
    assert mutate or 4 * passed[0] == (4 * (T + 2) if three else 4 * (3 * T + 3))
    return s


def back_steps(T):
    s = []
    for r in range(T):
        s.append(("wait", "wready", 4 * (r + 1)))
        s.append(("read", "GA%d" % (r & 1), None))  # the W rows of tile r (cold paths read them again: the same accesses)
        s.append(("read", "GB%d" % (r & 1), None))
        s.append(("read", "Mb%d" % (r & 3), None))  # (heavy rows)
        s.append(("arrive", "digdone", 4))
        s.append(("read", "Mb%d" % ((r + 3) & 3), None))  # the contraction of a group: the slots of both its tiles
        s.append(("read", "Mb%d" % (r & 3), None))
        s.append(("arrive", "itdone", 4))
    return s


class Race(Exception):
    pass


class Deadlock(Exception):
    pass


def run(T, rng, mutate=None, variant="shipped"):
    prog = [front_steps(w, T, mutate, variant) for w in range(NF)] + [back_steps(T)]
    pc = [0] * NAG
    clock = [[0] * NAG for _ in range(NAG)]
    for a in range(NAG):
        clock[a][a] = 1
    count, cclock = {}, {}
    last_write = {}  # region -> list of (agent, part, stamp)
    reads = {}       # region -> list of (agent, part, stamp) since they were last ordered in front of a write
    weight = [rng.choice((1, 1, 1, 3, 10, 40)) for _ in range(NAG)]  # some waves run far ahead of the others

    def ordered(b, stamp, a):  # the access (b, stamp) happens before agent a's present
        return clock[a][b] >= stamp

    def overlap(p, q):
        return p is None or q is None or p == q

    live = [a for a in range(NAG) if prog[a]]
    while live:
        runnable = []
        for a in live:
            st = prog[a][pc[a]]
            if st[0] != "wait" or count.get(st[1], 0) >= st[2]:
                runnable.append(a)
        if not runnable:
            raise Deadlock((T, [(a, pc[a], prog[a][pc[a]]) for a in live], dict(count)))
        a = rng.choices(runnable, [weight[x] for x in runnable])[0]
        for _ in range(rng.randint(1, 6)):
            st = prog[a][pc[a]]
            kind = st[0]
            if kind == "wait":
                if count.get(st[1], 0) < st[2]:
                    break
                cc = cclock[st[1]]
                ca = clock[a]
                for i in range(NAG):
                    if cc[i] > ca[i]:
                        ca[i] = cc[i]
            elif kind == "arrive":
                count[st[1]] = count.get(st[1], 0) + st[2]
                cc = cclock.setdefault(st[1], [0] * NAG)
                ca = clock[a]
                for i in range(NAG):
                    if ca[i] > cc[i]:
                        cc[i] = ca[i]
                ca[a] += 1
            else:
                region, part = st[1], st[2]
                stamp = clock[a][a]
                for (b, q, t) in last_write.get(region, ()):
                    if b != a and overlap(part, q) and not ordered(b, t, a):
                        raise Race((T, kind, region, "agent %d step %d" % (a, pc[a]), "against the write of agent %d" % b))
                if kind == "write":
                    for (b, q, t) in reads.get(region, ()):
                        if b != a and overlap(part, q) and not ordered(b, t, a):
                            raise Race((T, kind, region, "agent %d step %d" % (a, pc[a]), "against the read of agent %d" % b))
                    reads[region] = [x for x in reads.get(region, ()) if not overlap(part, x[1])]
                    last_write[region] = [x for x in last_write.get(region, ()) if not overlap(part, x[1])] + [(a, part, stamp)]
                else:
                    rl = reads.setdefault(region, [])
                    rl[:] = [x for x in rl if not (x[0] == a and x[1] == part)]
                    rl.append((a, part, stamp))
            pc[a] += 1
            if pc[a] == len(prog[a]):
                live.remove(a)
                break
    return count


TILES = [0, 1, 2, 3, 4, 5, 9]
SCHEDULES = 450  # per tile count: 3 150 in all


@pytest.mark.parametrize("T", TILES)
def test_no_schedule_deadlocks_or_races(T):
    rng = random.Random(1000 + T)
    want = {c: v for c, v in closed_forms(T).items() if v}
    for _ in range(SCHEDULES):
        assert run(T, rng) == want


@pytest.mark.parametrize("T", TILES)
def test_the_hand_offs_not_kept_are_safe_too(T):
    rng = random.Random(2000 + T)
    want = {c: v for c, v in closed_forms(T, "three").items() if v}
    for _ in range(SCHEDULES // 3):
        assert run(T, rng, variant="three") == want


@pytest.mark.parametrize("T", [0, 1, 2])
def test_ledger_walk(T):
    """The walk of the ledger for workgroups of 0, 1 and 2 tiles: every wait's target is reached by exactly the adds the ledger
    names, in program order per agent -- the largest target of each counter equals the counter's final value, so no waiter asks
    for an add that never comes and no add is left over that a later wait could mistake for its own."""
    prog = [front_steps(w, T) for w in range(NF)] + [back_steps(T)]
    adds, largest = {}, {}
    for steps in prog:
        for st in steps:
            if st[0] == "arrive":
                adds[st[1]] = adds.get(st[1], 0) + st[2]
            elif st[0] == "wait":
                largest[st[1]] = max(largest.get(st[1], 0), st[2])
    assert adds == {c: v for c, v in closed_forms(T).items() if v}
    for c, t in largest.items():
        assert t <= adds[c], (c, t, adds[c])
    for c in ("fbar", "solved", "wready", "cbar"):
        if c in adds:
            assert largest[c] == adds[c], c
    # the extra trip has no solver and no P4a: no wait on solved behind the last tile's
    for steps in prog[:NF]:
        assert all(st[2] <= T for st in steps if st[0] == "wait" and st[1] == "solved")


@pytest.mark.parametrize("mutate,variant,exc", [("no-solved-wait", "shipped", Race), ("no-f3", "shipped", Race),
                                                ("solved-target", "shipped", Deadlock), ("no-xfree-wait", "three", Race)])
def test_the_model_sees_a_broken_protocol(mutate, variant, exc):
    """The checker is not vacuous: without the wait for the solver, or with nothing between P4a and the x~ stores of the staging,
    some schedule races; with a target one trip too high every schedule deadlocks."""
    rng = random.Random(7)
    with pytest.raises(exc):
        for _ in range(200):
            run(3, rng, mutate, variant)
