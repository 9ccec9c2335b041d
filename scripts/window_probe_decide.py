"""The decision rule over scripts/native/window_probe.hip's records (profiles/window_probe.jsonl):
a residency cap is a gain only if
  * on every allocation draw its median is below the uncapped (cap 0) median by more than twice
    the noise yardstick, the spread (max - min) of cap 0's round medians on that draw, and
  * the best cap is the same or adjacent (in the probe's list of caps) on all draws.
A cap whose residency equals the uncapped one (the occupancy API's figure) is the uncapped kernel
with an LDS request: it is listed but cannot win. Prints one JSON record.

    python scripts/window_probe_decide.py profiles/window_probe.jsonl
"""
import json
import sys


def decide(records):
    draws = sorted({r["draw"] for r in records})
    caps = sorted({r["cap"] for r in records if "median_ms" in r})
    by = {(r["draw"], r["cap"]): r for r in records if "median_ms" in r}
    uncapped_res = by[(draws[0], 0)]["resident_wg_per_cu"]
    real = [c for c in caps if c and by[(draws[0], c)]["resident_wg_per_cu"] < uncapped_res]
    per_draw, best = [], []
    for d in draws:
        u = by[(d, 0)]
        spread = max(u["round_median_ms"]) - min(u["round_median_ms"])
        med = {c: by[(d, c)]["median_ms"] for c in caps}
        b = min(real, key=lambda c: med[c]) if real else None
        best.append(b)
        per_draw.append({"draw": d, "uncapped_ms": u["median_ms"], "uncapped_round_spread_ms": round(spread, 4),
                         "median_ms": med, "best_cap": b,
                         "beats_uncapped_by_2x_spread": [c for c in real if u["median_ms"] - med[c] > 2 * spread]})
    winners = set(real)
    for p in per_draw:
        winners &= set(p["beats_uncapped_by_2x_spread"])
    pos = [real.index(b) for b in best if b is not None]
    adjacent = bool(pos) and max(pos) - min(pos) <= 1
    gain = bool(winners) and adjacent
    win = min(winners, key=lambda c: sum(p["median_ms"][c] for p in per_draw)) if gain else None
    return {"uncapped_resident_wg_per_cu": uncapped_res, "caps_below_uncapped": real, "per_draw": per_draw,
            "caps_winning_on_every_draw": sorted(winners), "best_caps_adjacent": adjacent, "gain": gain,
            "winning_cap": win}


def main():
    with open(sys.argv[1]) as f:
        records = [json.loads(line) for line in f if line.strip()]
    print(json.dumps(decide([r for r in records if "draw" in r])))


if __name__ == "__main__":
    main()
