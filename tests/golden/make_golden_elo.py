#!/usr/bin/env python3
"""Generate tests/golden/g20_elo.npz: the ratings the REAL reference's `Elo` (src/utils.py) holds after every update of
three result sequences.

Run in the build container only (needs the reference checkout; CPU, no GPU, no compiled piece):

    python tests/golden/make_golden_elo.py             # AZ_REFERENCE=<checkout> if it is not /root/reference

src/utils.py is imported unmodified from the checkout by file path.  Per start pair - (1500, 1500), (1700, 1500) and
(1500, 1900); the last one holds rating A on the floor of 1500 whenever it loses - 64 results drawn from {1, 0.5, 0}
with a seeded generator go through `Elo.update` one by one, and both ratings are recorded after each.  Recorded:

    starts   float64 [3, 2]      results  float64 [3, 64]      ratings  float64 [3, 64, 2]

Nothing from the reference is copied: the committed output is data.
"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("AZ_REFERENCE", "/root/reference")
STARTS = ((1500, 1500), (1700, 1500), (1500, 1900))
N = 64


def main():
    spec = importlib.util.spec_from_file_location("ref_utils", os.path.join(REF, "src", "utils.py"))
    utils = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(utils)
    rng = np.random.default_rng(20)
    results = rng.choice(np.array([1.0, 0.5, 0.0]), size=(len(STARTS), N))
    ratings = np.zeros((len(STARTS), N, 2))
    for i, (a, b) in enumerate(STARTS):
        elo = utils.Elo(a, b)
        for j in range(N):
            r = float(results[i, j])
            ratings[i, j] = elo.update(1 if r == 1.0 else r)       # the scores update_elo passes: 1, 0.5, 0
    assert (ratings[2, :, 0] == 1500).any() and (ratings[1, :, 1] == 1500).any()      # both floors are met
    np.savez(os.path.join(HERE, "g20_elo.npz"), starts=np.array(STARTS, np.float64), results=results, ratings=ratings)
    print("wrote g20_elo.npz", ratings[:, -1].tolist())


if __name__ == "__main__":
    main()
