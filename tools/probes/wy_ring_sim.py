"""The dy / h staging ring of the dWhy sums in k_bwd_scatter (csrc/persistent.hip), with the waves of one workgroup running
asynchronously -- what ring_protocol_sim.py, which advances everything in lock step, does not model.

Wave 11 (the stager) leaves the operands of step tu in slot tu % 3 of a three-deep LDS ring and announces S - tu in s_wy; each
of the eight product waves, behind its two products of step t, fetches slot t % 3 into registers (after s_wy >= S - t) and
releases it by adding to a count.  Before it stages step tu over what slot tu % 3 held (step tu + 3), the stager waits for
that count.  What the product waves may do relative to each other comes from the recurrence: the products of step t need
dg_t, which needs the partial sums Q_{t+1} of every workgroup, which needed this workgroup's Q_{t+2} from every one of its
product waves -- so a wave can start the products of step t once ALL waves have finished the products of step t + 2, whatever
they have done of the dWhy share that comes behind those products.  A wave can therefore be up to two steps ahead of another.

count = "slot": one count per slot, the stager waits for 8 * (earlier uses of the slot)            (the kernel)
count = "ring": one running count, the stager waits for 8 * (S - tu - 3)                           (the kernel until this was found)
With the running count the releases a fast wave makes for steps tu + 2 and tu + 1 stand in for the release a slow wave has
not made for step tu + 3: the slot is staged over before the slow wave has read it, and that wave multiplies the operands of
step tu where it should have had those of step tu + 3.

run() returns None, or the first wrong fetch as (wave, step wanted, step found)."""
import random


def run(S, count="slot", laggard=None, seed=None, waves=8):
    prog = []
    for t in range(S - 1, 1, -1):
        prog += [("prod", t), ("fetch", t), ("release", t)]
    prog += [("fetch", 1), ("release", 1)]
    pc = [0] * waves
    prod_done = [S] * waves          # lowest step whose products the wave has finished (S: none yet)
    slot, staged = [None] * 3, 0     # ring content; s_wy
    ring_count, slot_count = 0, [0, 0, 0]
    st = {"tu": S - 1}
    rng = random.Random(seed)

    def stager_enabled():
        tu = st["tu"]
        if tu < 1:
            return False
        # wave 11 is at most four steps ahead of the chain (s_stage): step tu + 4 finished elementwise, which needed Q_{tu+5}
        # of every workgroup, which needed this workgroup's Q_{tu+6} from every product wave
        if tu + 6 <= S - 1 and max(prod_done) > tu + 6:
            return False
        if tu + 3 > S - 1:
            return True
        if count == "slot":
            return slot_count[tu % 3] >= waves * ((S - 1 - tu) // 3)
        return ring_count >= waves * (S - tu - 3)

    def wave_enabled(w):
        if pc[w] >= len(prog):
            return False
        op, t = prog[pc[w]]
        if op == "prod":
            return t + 2 > S - 1 or max(prod_done) <= t + 2
        if op == "fetch":
            return staged >= S - t
        return True

    while True:
        actors = [a for a in range(-1, waves) if (stager_enabled() if a < 0 else wave_enabled(a))]
        if not actors:
            assert all(p == len(prog) for p in pc) and st["tu"] == 0, ("deadlock", S, count, pc, st)
            return None
        if seed is not None:
            a = rng.choice(actors)
        else:  # the other waves as far as they can go (the one furthest behind first), then the stager; the laggard only
            # when nothing else can move
            others = sorted((pc[x], x) for x in actors if x >= 0 and x != laggard)
            a = others[0][1] if others else -1 if -1 in actors else laggard
        if a < 0:
            tu = st["tu"]
            slot[tu % 3], staged = tu, S - tu
            st["tu"] = tu - 1
            continue
        op, t = prog[pc[a]]
        pc[a] += 1
        if op == "prod":
            prod_done[a] = t
        elif op == "fetch":
            if slot[t % 3] != t:
                return (a, t, slot[t % 3])
        else:
            ring_count += 1
            slot_count[t % 3] += 1


if __name__ == "__main__":
    for S in range(2, 120):
        for lag in range(8):
            assert run(S, "slot", laggard=lag) is None, (S, lag)
        for seed in range(20):
            assert run(S, "slot", seed=seed) is None, (S, seed)
    bad = run(20, "ring", laggard=4)
    print("dy / h ring of k_bwd_scatter: one count per slot is consistent for S = 2..119 under laggard and random schedules;")
    print(f"one running count, S = 20, wave 4 slow: wave {bad[0]} wanted step {bad[1]} and found step {bad[2]}")
