"""The numpy reference of a Generations rule (B/S/C) on one board: what tests/test_gpu_generations.py checks the GPU
against.  tests/test_generations_host.py pins it to tests/rule_reference.py at 2 states.

A cell's state is s in 0 .. nstates - 1: 0 dead, 1 alive, above dying; n = its neighbours in state 1.
s = 0 -> 1 if bit n of birth else 0;  s = 1 -> 1 if bit n of survive, else 2 (nstates > 2) or 0;  s >= 2 -> s + 1 if
s + 1 < nstates else 0.  boundary 0 = torus, 1 = bounded (outside is state 0 forever and no cell of the board)."""
import numpy as np


def masks(rule):
    """(birth, survive, nstates) of "B2/S345/C4" / "B3/S23" (canonical text only)."""
    f = rule.upper().split("/")
    assert f[0][0] == "B" and f[1][0] == "S", rule
    n = int(f[2].lstrip("CG")) if len(f) > 2 else 2
    return sum(1 << int(d) for d in f[0][1:]), sum(1 << int(d) for d in f[1][1:]), n


def gen_step(states, birth, survive, nstates, boundary, generations):
    """`generations` synchronous generations of a (H, W) uint8 board of states."""
    s = np.asarray(states).astype(np.uint8)
    birth_t = np.array([(birth >> n) & 1 for n in range(9)], dtype=np.uint8)
    survive_t = np.array([(survive >> n) & 1 for n in range(9)], dtype=np.uint8)
    h, w = s.shape
    for _ in range(generations):
        a = (s == 1).astype(np.uint8)
        if boundary == 0:
            n = sum(np.roll(np.roll(a, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx)
        else:
            p = np.zeros((h + 2, w + 2), dtype=np.uint8)
            p[1:-1, 1:-1] = a
            n = sum(p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx)
        died = 2 if nstates > 2 else 0
        nxt = np.where(s == 0, birth_t[n], np.where(s == 1, np.where(survive_t[n] != 0, 1, died),
                                                    np.where(s + 1 < nstates, s + 1, 0)))
        s = nxt.astype(np.uint8)
    return s


def gen_cycles(states, birth, survive, nstates, boundary, max_generations):
    """(transient, period, state-1 cells of B_transient) by brute force: t* = the smallest t >= 1 with B_t = B_s for
    some s < t, resolved when t* <= max_generations; (-1, 0, 0) otherwise."""
    s = np.asarray(states).astype(np.uint8)
    seen = {s.tobytes(): (0, int((s == 1).sum()))}
    for t in range(1, max_generations + 1):
        s = gen_step(s, birth, survive, nstates, boundary, 1)
        k = s.tobytes()
        if k in seen:
            mu, pop = seen[k]
            return mu, t - mu, pop
        seen[k] = (t, int((s == 1).sum()))
    return -1, 0, 0


def stacked(states, nstates):
    """The (nstates - 1) H x W board whose rows [(k - 1) H, k H) are the indicator of state k."""
    s = np.asarray(states)
    return np.concatenate([(s == k).astype(np.uint8) for k in range(1, nstates)], axis=0)


def gen_hash(states, nstates, oracle):
    """The batch's hash of a state board: oracle.board_hash of the stacked board."""
    return oracle.board_hash(stacked(states, nstates))
