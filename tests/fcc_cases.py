"""The corpus on which the upstream find_chessboard_corners.cc (oracle/_ref, built by `make -C oracle ref`), the C
restatement (oracle/mrgingham_oracle.c) and the HIP kernels are compared with one another: the hand-built responses of
cc_cases.py, random sparse responses, small images -- and the known answers of upstream on a part of it that travel
with the repository (tests/golden/fcc_kat.npz, written by tests/golden/make_fcc_golden.py).

Shared by tests/test_oracle_fcc.py (CPU), tests/test_gpu_fcc_reference.py (GPU) and make_fcc_golden.py."""
import json
import os

import numpy as np

import cc_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fcc_kat.npz")

DETECT_LEVELS = (0, 1, 3)          # on responses the level only scales the output (:319, :346, :369, :390)


def response_detect_cases():
    """-> [(name, response, level image, level, hand-derived expectation or None)]: every detect case of cc_cases at
    level 0, a few of them at levels 1 and 3 as well, and the large frames."""
    out = []
    for name, d, img, expected in cc_cases.detect_cases() + cc_cases.large_detect_cases():
        out.append((name, d, img, 0, expected))
    for name, d, img, expected in cc_cases.detect_cases():
        if name.startswith(("two pixels", "three blobs", "peak 32767: 2048", "208-pixel")):
            for level in DETECT_LEVELS[1:]:
                out.append((f"{name} @ level {level}", d, img, level, None))
    return out


def response_refine_cases():
    """-> [(name, points, levels, response, level image, level, hand-derived expectation or None)]"""
    return list(cc_cases.refine_cases())


def random_refine_points(rng, d, level, k=60):
    """Points about the hot pixels of `d` in full-resolution coordinates, some twice, some nowhere near, some
    outside; tags level+1 mostly, some level+2 and level (not refinable)."""
    ys, xs = np.nonzero(d > 15)
    sel = rng.choice(len(xs), size=k, replace=True)
    scale = float(1 << level)
    h, w = d.shape
    pts = np.stack([(xs[sel] + rng.uniform(-1.6, 1.6, k) + 0.5) * scale - 0.5,
                    (ys[sel] + rng.uniform(-1.6, 1.6, k) + 0.5) * scale - 0.5], axis=1)
    pts = np.concatenate([pts, pts[:8], [[-5.0, -5.0], [w * scale + 3, h * scale + 3], [0.0, 0.0]]])
    lv = np.full(len(pts), level + 1, np.int8)
    lv[::7] = level + 2
    lv[3::11] = level
    return pts, lv


def zero_ring(d):
    """The response as the upstream pipeline can produce it: the 7-pixel frame is never written (:506, ChESS.c:62-63).
    mrgingham_amd_cc_on_response_batch documents that it clears the frame of what it is given; comparisons with the
    device hand the reference the same."""
    out = np.zeros_like(d)
    out[7:-7, 7:-7] = d[7:-7, 7:-7]
    return out


def random_sparse_batch(shape, nblobs, noise, B=4):
    """Frames as test_gpu_cc_rules.test_random_sparse_responses builds them (same generator, same images)."""
    h, w = shape
    rng = np.random.RandomState(h * 1009 + w)
    ds = [cc_cases.random_sparse_response(rng, h, w, nblobs, noise) for _ in range(B)]
    imgs = [cc_cases.flat_img(h, w) if f % 3 else rng.randint(0, 256, size=(h, w)).astype(np.uint8) for f in range(B)]
    imgs[1] = (rng.randint(0, 40, size=(h, w)) + 100).astype(np.uint8)      # low variance: sigma ~ 11.5 < 20
    return ds, imgs


def small_images():
    """Images of 131x96 or smaller, for the known-answer file and the smallest GPU size."""
    from mrgingham_amd import synth
    checker = (((np.arange(48).reshape(-1, 1) // 3 + np.arange(64).reshape(1, -1) // 3) & 1) * 200 + 20).astype(np.uint8)
    return {
        "board4_131x96": synth.board_frame(131, 96, 4, 1).numpy(),
        "cluttered4_131x96": synth.cluttered_board_frame(131, 96, 4, 2).numpy(),
        "noise_smooth1_96x64": synth.noise_frame(96, 64, 3, smooth=1).numpy(),
        "checker3px_64x48": checker,
    }


# ----------------------------------------------------------------------------- the known-answer file

def save_kat(path, entries):
    """entries: [(meta dict of plain values, {field: array})]"""
    arrays = {"manifest": np.frombuffer(json.dumps([m for m, _ in entries]).encode(), np.uint8)}
    for i, (_, fields) in enumerate(entries):
        for k, v in fields.items():
            arrays[f"{i}.{k}"] = np.asarray(v)
    np.savez_compressed(path, **arrays)


def load_kat(path=GOLDEN):
    z = np.load(path)
    manifest = json.loads(z["manifest"].tobytes().decode())
    out = []
    for i, meta in enumerate(manifest):
        prefix = f"{i}."
        out.append((meta, {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix)}))
    return out
