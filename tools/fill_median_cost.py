"""Cost of a FillMedian fit over the continuous columns of the headline frame: 13 float64 columns
of 45 M rows, through kernels_select.select_median_many (what FillMedian.fit_end runs).

    python tools/fill_median_cost.py [--rows 45000000] [--cols 13] [--out FILE.json]

Three data shapes, each timed with the candidate path allowed and switched off (the same columns
then take all six full passes):
  bits     uniform over the finite float64 bit patterns: ~rows / 2048 keys per top-digit bin, the
           candidate path's case
  unit     uniform(0, 1): half of the rows share the median's top-digit bin -> full passes
  zeros    60 % zeros, the rest uniform(0, 1000): zero-inflated counts -> full passes
Prints one JSON line (milliseconds per fit: median of 5 after 2 warm-up fits; bytes per full pass).

The consistency check the select has to meet is made here: the `bits` shape must take the
candidate path on every column, and its fit must then be faster than the same columns through all
the full passes.  The exit status is 1 when it does not."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from nvtabular_amd import kernels_select as KS


def make(kind, rows, gen):
    if kind == "bits":
        x = torch.randint(-2**63, 2**63 - 1, (rows,), dtype=torch.int64, device="cuda", generator=gen).view(torch.float64)
        x[~torch.isfinite(x)] = 0.0
        return x
    x = torch.rand(rows, dtype=torch.float64, device="cuda", generator=gen)
    if kind == "zeros":
        x = x * 1000.0
        x[torch.rand(rows, device="cuda", generator=gen) < 0.6] = 0.0
    return x


def timed(chunks, allow):
    ms = []
    for i in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = KS.select_median_many(chunks, allow_candidates=allow)   # (ends with its read-back)
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(ms[2:])
    return ms[len(ms) // 2], sorted({r.path for r in res}), [r.median for r in res[:2]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=45_000_000)
    ap.add_argument("--cols", type=int, default=13)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    rec = {"rows": a.rows, "cols": a.cols, "bytes_per_full_pass": a.rows * a.cols * 8, "shapes": {}}
    for kind in ("bits", "unit", "zeros"):
        cols = [make(kind, a.rows, gen) for _ in range(a.cols)]
        chunks = [[(c, None, None)] for c in cols]
        ms_c, paths_c, med_c = timed(chunks, True)
        ms_f, paths_f, med_f = timed(chunks, False)
        assert med_c == med_f, (kind, med_c, med_f)
        rec["shapes"][kind] = {"ms_candidates_allowed": round(ms_c, 3), "paths": paths_c,
                               "ms_full_passes": round(ms_f, 3), "paths_forced": paths_f}
        del cols, chunks
    bits = rec["shapes"]["bits"]
    rec["candidate_path_taken"] = bits["paths"] == [KS.PATH_CAND] and bits["paths_forced"] == [KS.PATH_FULL]
    rec["candidate_path_faster"] = bits["ms_candidates_allowed"] < bits["ms_full_passes"]
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not rec["candidate_path_taken"]:
        sys.exit("FAILED: the columns of uniform bit patterns did not take the candidate path")
    if not rec["candidate_path_faster"]:
        sys.exit("FAILED: the candidate path is not faster than the full passes on the same columns")


if __name__ == "__main__":
    main()
