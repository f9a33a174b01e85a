#!/usr/bin/env python3
"""Writes tests/golden/fcc_kat.npz: inputs AND the outputs of the upstream find_chessboard_corners.cc on them.

Runs only where the reference build exists (oracle/_ref/libfcc_ref.so and libfcc_resp_ref.so, `make -C oracle ref`
with the reference tree present).  Run from the repository root:

    python tests/golden/make_fcc_golden.py

The corpus (tests/fcc_cases.py): every hand-built response case of tests/cc_cases.py -- detection and refinement --
and a few images of 131x96 or smaller with their level images, detection at levels 0..3, every refine step and the
chains from start levels 1..3.  Inputs are stored, not regenerated, so a generator that drifts cannot move the
answers.  tests/test_oracle_fcc.py replays the file through the restatement (never skipped) and checks it against
the live reference build (skipped where that is absent).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import oracle  # noqa: E402
import fcc_cases  # noqa: E402

LIMIT = 128 * 1024


def entries():
    out = []
    for name, d, img, level, _ in fcc_cases.response_detect_cases():
        out.append(({"kind": "detect_on_response", "name": name, "level": level},
                    {"d": d, "img": img, "out": oracle.ref_cc_detect_on_response(d, img, level)}))
    for name, pts, lv, d, img, level, _ in fcc_cases.response_refine_cases():
        p2, l2, n = oracle.ref_cc_refine_on_response(pts, lv, d, img, level)
        out.append(({"kind": "refine_on_response", "name": name, "level": level, "n": int(n)},
                    {"pts": pts, "lv": lv, "d": d, "img": img, "out_pts": p2, "out_lv": l2}))
    for name, image in fcc_cases.small_images().items():
        out.append(({"kind": "image", "name": name}, {"image": image}))
        levels = {L: oracle.decimate(image, L) for L in (1, 2, 3)}
        for L, li in levels.items():
            out.append(({"kind": "level_image", "name": name, "level": L}, {"image": li}))
        found = {}
        for L in range(4):
            found[L] = oracle.ref_find_corners(image, L, levels.get(L))
            out.append(({"kind": "detect", "name": name, "level": L}, {"out": found[L]}))
        for L in range(3):
            pts = found[L + 1].astype(np.float64) / 1000.0
            lv = np.full(len(pts), L + 1, np.int8)
            p2, l2, n = oracle.ref_refine_corners(pts, lv, image, L, levels.get(L))
            out.append(({"kind": "refine", "name": name, "level": L, "n": int(n)},
                        {"pts": pts, "lv": lv, "out_pts": p2, "out_lv": l2}))
        for start in (3, 2, 1):
            p, l = oracle.ref_chain(image, start, levels)
            out.append(({"kind": "chain", "name": name, "start": start}, {"out_pts": p, "out_lv": l}))
    return out


def main():
    assert oracle.have_reference_fcc(), "oracle/_ref is not built: run `make -C oracle ref` where the reference tree is"
    e = entries()
    path = os.path.join(HERE, "fcc_kat.npz")
    fcc_cases.save_kat(path, e)
    size = os.path.getsize(path)
    kinds = {}
    for m, _ in e:
        kinds[m["kind"]] = kinds.get(m["kind"], 0) + 1
    print(f"wrote {path}: {size} bytes, {kinds}")
    assert size <= LIMIT, size


if __name__ == "__main__":
    main()
