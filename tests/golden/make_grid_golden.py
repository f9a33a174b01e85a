#!/usr/bin/env python3
"""Writes tests/golden/grid_kat.npz: the answers of the upstream find_grid.cc on the cases of tests/grid_cases.py.

Runs only where the reference build exists (oracle/_ref/libgrid_ref.so, `make -C oracle ref` with the reference tree
present).  Run from the repository root:

    python tests/golden/make_grid_golden.py

Per case the file holds the name, gridn, a hash of the generated input (so that a generator that drifts is caught, not
followed), and upstream's answer with every neighbour ring at the canonical start (oracle/ref_stub/boost/polygon/
voronoi.hpp): a found flag and, per corner of a found board, the index of the input point -- upstream's outputs are
input points divided by 1000.  The inputs themselves are regenerated from seeds by tests/grid_cases.py.
tests/test_oracle_grid.py replays the file through the product (never skipped) and checks it against the live
reference build (skipped where that is absent).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import oracle  # noqa: E402
import grid_cases  # noqa: E402

LIMIT = 291 * 1000          # the largest fixture there is


def main():
    assert oracle.have_reference_grid(), "oracle/_ref is not built: run `make -C oracle ref` where the reference tree is"
    names, gridns, hashes, found, offsets, indices = [], [], [], [], [0], []
    for name, gridn, pts, _ in grid_cases.all_cases(HERE):
        board = oracle.ref_find_grid(pts, gridn, 0)
        names.append(name)
        gridns.append(gridn)
        hashes.append(grid_cases.input_hash(gridn, pts))
        found.append(board is not None)
        if board is not None:
            idx = grid_cases.indices_of(board, pts)
            assert np.array_equal(grid_cases.board_of(idx, pts), board), name
            indices.append(idx)
        offsets.append(offsets[-1] + (gridn * gridn if board is not None else 0))
    assert len(set(names)) == len(names)
    path = os.path.join(HERE, "grid_kat.npz")
    np.savez_compressed(path, names=np.array(names), gridn=np.array(gridns, np.int16), hash=np.array(hashes, np.uint64),
                        found=np.array(found, np.bool_), offsets=np.array(offsets, np.int32),
                        indices=np.concatenate(indices).astype(np.int16))
    size = os.path.getsize(path)
    print(f"wrote {path}: {size} bytes, {len(names)} cases, {int(np.sum(found))} boards")
    assert size <= LIMIT, size


if __name__ == "__main__":
    main()
