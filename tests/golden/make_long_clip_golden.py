#!/usr/bin/env python3
"""Long-clip full-size golden from the fp32 CPU ORACLE (oracle/unet.py, generic in T).  Run on the CPU, once:

    python tests/golden/make_long_clip_golden.py          # -> tests/golden/long_clip_oracle.npz

Case (tests/long_clip_cases.py holds the seeds and the sampling positions):
  unet_y       one UNet forward at T = 32, B = 1, t = 601, context 77 + 256 (shared image tokens)   (sampled positions)
  unet_y_norm  its L2 norm                                                                          (whole tensor)
"""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import long_clip_cases as lc  # noqa: E402
from conftest import sub_state_dict  # noqa: E402
from oracle import unet as ounet  # noqa: E402


def main():
    torch.set_num_threads(os.cpu_count() or 1)
    t0 = time.time()
    inp = lc.inputs()
    usd = sub_state_dict(lc.full_state_dict(("model.diffusion_model.",)), "model.diffusion_model.")
    print(f"[{time.time() - t0:6.0f}s] UNet weights ready", flush=True)
    with torch.no_grad():
        y = ounet.unet_forward(usd, lc.UNET_CFG, torch.cat([inp["x_T"], inp["c_concat"]], 1), torch.tensor([lc.UNET_T]),
                               inp["cond"], inp["fs"])
    flat = y.reshape(-1)
    out = {"unet_y": flat[lc.sample_idx(flat.numel(), lc.N_OUT, 3)].numpy(),
           "unet_y_norm": np.float64(float(y.double().norm())),
           "unet_y_shape": np.array(y.shape, dtype=np.int64)}
    print(f"[{time.time() - t0:6.0f}s] unet_y {tuple(y.shape)} std {float(y.std()):.4f}", flush=True)
    np.savez_compressed(lc.GOLDEN_FILE, **out)
    print(f"wrote {lc.GOLDEN_FILE} ({os.path.getsize(lc.GOLDEN_FILE) / 1e6:.2f} MB)")


if __name__ == "__main__":
    main()
