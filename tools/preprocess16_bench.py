"""Timing of the 16-bit batch preprocessing (mrgingham_amd_preprocess16_batch) on 64 frames of 4096x3072.

python tools/preprocess16_bench.py [calls [data class]]

Two data classes: a 12-bit board (R = smax - smin + 1 ~ 4 K: slabs of 16-bit LDS counters) and full-range 16-bit noise
(R = 65 536: whole tiles in four parts of 16 384 32-bit LDS counters, the tile read once per part).  Per case: ms per batch, the bytes-per-pixel model of the schedule, the fraction of the
8 TB/s HBM peak that model moves in that time, and the engine clock the blend launches ran at (Detector.sclk_mhz); the
same for option preprocess_fused 0 (the one-image kernels).  One JSON line per case."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import mrgingham_amd
from mrgingham_amd import synth

W, H, B = 4096, 3072, 64
HBM_PEAK = 8e12
N = int(sys.argv[1]) if len(sys.argv) > 1 else 20


def model_bytes_per_px(fused, clahe, blur, hist_reads):
    """Algorithmic traffic of the schedule (tables excluded); hist_reads = reads of the frame by the histogram pass."""
    if fused:
        # extrema 2 + histograms 2 per read + blend 2 + 1 written; without CLAHE the last pass alone
        return ((2 + 2 * hist_reads + 3) if clahe else 3) + (2 if blur > 1 else 0)
    # one-image kernels: extrema 2, normalise 2 + 2, histogram 2, blend 2 + 1, blur 1 + 1
    return ((11 if clahe else 3) + (2 if blur else 0))


def main():
    det = mrgingham_amd.Detector(0)
    g = torch.Generator(device="cuda").manual_seed(1)
    board = synth.board_batch(4, W, H, 10, 0, device="cuda").repeat(B // 4, 1, 1).to(torch.int32)
    classes = {
        "board12": (board * 16 + 1000).to(torch.int16).view(torch.uint16).contiguous(),
        "full16": torch.randint(-32768, 32768, (B, H, W), generator=g, device="cuda", dtype=torch.int16).view(torch.uint16),
    }
    del board
    det.set_kernel_timing(2)  # the engine-clock probe alone
    only = sys.argv[2] if len(sys.argv) > 2 else None
    for name, frames in classes.items():
        if only and name != only:
            continue
        for fused in (1, 0):
            det.set_option("preprocess_fused", fused)
            for clahe, blur in [(True, 1), (True, 0)]:
                for _ in range(3):
                    det.preprocess(frames, clahe=clahe, blur_radius=blur)
                torch.cuda.synchronize()
                det.sclk_mhz()  # (resets the probe's counters)
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(N):
                    det.preprocess(frames, clahe=clahe, blur_radius=blur)
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / N
                bpp = model_bytes_per_px(fused, clahe, blur, 1 if name == "board12" else 4)
                print(json.dumps({"data": name, "preprocess_fused": fused, "clahe": clahe, "blur": blur, "frames": B,
                                  "ms": round(ms, 3), "model_B_per_px": bpp,
                                  "hbm_fraction": round(bpp * B * W * H / (ms * 1e-3) / HBM_PEAK, 3),
                                  "sclk_mhz": round(det.sclk_mhz(), 1)}), flush=True)
    det.close()


if __name__ == "__main__":
    main()
