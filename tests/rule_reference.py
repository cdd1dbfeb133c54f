"""The numpy reference stepper of a life-like rule on one board: what tests/test_gpu_board_rules.py checks the GPU
against.  tests/test_board_rules_host.py pins it to the CPU oracle (oracle/gol_oracle.py) under B3/S23."""
import numpy as np


def masks(rule):
    """(birth, survive) of "B36/S23" (canonical text only) or of a pair of masks."""
    if not isinstance(rule, str):
        return int(rule[0]), int(rule[1])
    b, s = rule.upper().split("/")
    assert b[0] == "B" and s[0] == "S", rule
    return sum(1 << int(d) for d in b[1:]), sum(1 << int(d) for d in s[1:])


def ref_step(cells, birth, survive, boundary, generations):
    """`generations` synchronous generations of a (H, W) uint8 board under the rule; boundary 0 = torus, 1 = bounded
    (the cells outside are dead forever and are no cells of the board, also under a rule with B0)."""
    a = (np.asarray(cells) != 0).astype(np.uint8)
    birth_t = np.array([(birth >> n) & 1 for n in range(9)], dtype=np.uint8)
    survive_t = np.array([(survive >> n) & 1 for n in range(9)], dtype=np.uint8)
    h, w = a.shape
    for _ in range(generations):
        if boundary == 0:
            n = sum(np.roll(np.roll(a, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx)
        else:
            p = np.zeros((h + 2, w + 2), dtype=np.uint8)
            p[1:-1, 1:-1] = a
            n = sum(p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx)
        a = np.where(a != 0, survive_t[n], birth_t[n]).astype(np.uint8)
    return a


def soup(w, h, seed, fill=0.4):
    return (np.random.default_rng(seed).random((h, w)) < fill).astype(np.uint8)
