"""Records tests/golden/population_plan.json: what edt_slerp_population_layout and
edt_slerp_needed_table (host only, no GPU) answer over a seeded corpus of pair graphs. Run from
the repository root: python tests/golden/gen_population_plan.py <libedt_sync.so>

The library to record from is named on purpose: the fixture pins the plan against a build of the
commit BEFORE a change to the planner (build.build_library(out=...) at that commit), so the
script does not fall back to the library in the tree, which would compare the code with itself.

The named cases hold each path of the planner once; the seeded draws cover nmembers 1..10 and
0..20 children with self-pairs, duplicates and reversed pairs."""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.test_population_plan_cpu import FIXTURE, record  # noqa: E402


def named_cases():
    ring8 = [(c, (c + 1) % 8) for c in range(8)]
    k5 = [(a, b) for a in range(5) for b in range(a + 1, 5)]
    yield "two-member component", [(0, 1)], 2, 7
    yield "two-member component, reversed", [(1, 0)], 2, 7
    yield "two-member component, both orientations", [(0, 1), (1, 0)], 2, 7
    yield "3-cycle", [(0, 1), (1, 2), (2, 0)], 3, 100
    yield "3-cycle reversed", [(1, 0), (2, 1), (0, 2)], 3, 100
    yield "8-cycle", ring8, 8, 500
    yield "8-cycle reversed", [(b, a) for a, b in ring8], 8, 500
    yield "8-cycle and every reverse (16 children)", ring8 + [(b, a) for a, b in ring8], 8, 3
    yield "8-cycle, reverses and a self-pair (17 children)", ring8 + [(b, a) for a, b in ring8] + [(3, 3)], 8, 3
    yield "8 members, 4 chords fill the slots", ring8 + [(0, 2), (0, 3), (0, 4), (0, 5)], 8, 11
    yield "8 members, 5 chords: the triangle", ring8 + [(0, 2), (0, 3), (0, 4), (0, 5), (1, 3)], 8, 11
    yield "8 members, every pair: the triangle", [(a, b) for a in range(8) for b in range(a + 1, 8)][:20], 8, 11
    yield "K5: more chords than slots", k5, 5, 64
    yield "4 members, 3 chords of 2 slots", [(0, 1), (1, 2), (2, 3), (3, 0), (0, 2), (1, 3)], 4, 9
    yield ("5 members, 9 picked pairs of 8",
           [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0), (0, 2), (2, 0), (1, 3), (3, 1), (2, 4), (4, 2), (3, 0), (0, 3),
            (1, 1)], 5, 20)
    yield ("5 members, 8 picked pairs of 8",
           [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0), (0, 2), (2, 0), (1, 3), (3, 1), (2, 4), (4, 2), (3, 0), (0, 3)],
           5, 20)
    yield "16 duplicates of one pair", [(3, 6)] * 17, 8, 5          # the first + 16 extras: 17 children
    yield "15 duplicates of one pair", [(3, 6)] * 16, 8, 5
    yield "16 duplicates after the first, in 16 children", [(0, 1)] + [(1, 0)] * 15, 2, 5
    yield "17 of one self-pair", [(2, 2)] * 17, 3, 5
    yield "16 of one self-pair", [(2, 2)] * 16, 3, 5
    yield "self-pairs only, two components", [(4, 4), (2, 2)], 5, 1
    yield "two components", [(0, 1), (1, 2), (5, 6), (6, 7), (7, 5)], 8, 33
    yield "two components and a self-pair apart", [(0, 1), (2, 3), (3, 2), (7, 7)], 8, 33
    yield "a path of 9 distinct parents", [(m, m + 1) for m in range(8)], 9, 4
    yield "10 members, 10 distinct parents", [(m, (m + 1) % 10) for m in range(10)], 10, 4
    yield "10 members, 8 distinct parents", [(m + 2, (m + 1) % 8 + 2) for m in range(8)], 10, 4
    yield "9 members, 17 children, 9 distinct", [(m % 9, (m + 1) % 9) for m in range(17)], 9, 4
    yield "no children", [], 4, 10
    yield "no children, 9 members", [], 9, 10
    yield "no chunks", [(0, 1), (1, 2)], 3, 0
    yield "negative chunk count", [(0, 1), (1, 2)], 3, -1
    yield "member out of range", [(0, 1), (1, 9)], 8, 10
    yield "negative member", [(0, 1), (-1, 1)], 8, 10
    yield "member equal to the count", [(0, 3)], 3, 10
    yield "no members", [(0, 0)], 0, 10
    yield "negative member count", [], -1, 10
    yield "hub of 7 spokes", [(0, m) for m in range(1, 8)], 8, 12
    yield "hub of 7 spokes, reversed and doubled", [(m, 0) for m in range(1, 8)] * 2, 8, 12
    yield "20 children over 8 members", ring8 + ring8 + [(0, 4), (4, 0), (1, 5), (5, 5)], 8, 12


def drawn_cases(seed=20240607, per_cell=1):
    rng = random.Random(seed)
    for M in range(1, 11):
        for Q in list(range(0, 21)) * per_cell:
            live = rng.randint(1, M)                 # the parents the draw uses (others stay unused)
            pool = rng.sample(range(M), live)
            pairs = []
            while len(pairs) < Q:
                r = rng.random()
                if pairs and r < 0.15:
                    pairs.append(rng.choice(pairs))                  # a duplicate child
                elif pairs and r < 0.25:
                    a, b = rng.choice(pairs)
                    pairs.append((b, a))                             # a reversed pair
                elif r < 0.35:
                    a = rng.choice(pool)
                    pairs.append((a, a))                             # a self-pair
                else:
                    pairs.append((rng.choice(pool), rng.choice(pool)))
            if rng.random() < 0.03 and pairs:
                q = rng.randrange(len(pairs))
                pairs[q] = (pairs[q][0], M + rng.randint(0, 2))      # a member out of range
            yield f"draw M={M} Q={Q}", pairs, M, rng.choice([0, 1, 2, 17, 500, 100000])


def main():
    from evolutionarydistributedtraining_amd._lib import load_library
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    lib = load_library(sys.argv[1])
    cases = []
    for name, pairs, M, nch in list(named_cases()) + list(drawn_cases()):
        case = {"pairs": [list(p) for p in pairs], "nmembers": M, "nchunks": nch}
        cases.append({"name": name, "case": case, "want": record(case, lib)})
    with open(FIXTURE, "w") as f:
        f.write('{"cases": [\n' + ",\n".join(json.dumps(c, separators=(",", ":")) for c in cases) + "\n]}\n")
    print(len(cases), "cases,", os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
