#!/usr/bin/env python3
"""Writes tests/golden/ddim_step_bits.npz: the bits `HipOps.ddim_step` (tc_ddim_step / tc_ddim_step_eps) returns for the
operands of tests/test_gpu_multistep.py -- its seeded CPU draws, its `SC` / `_kw` scalars -- over par {v, eps} x guidance
{0, 2, 3} x rescale {0, 0.7} x noise {off, on} at each of its shapes.

The committed file was recorded on the MI355X at the last commit that had separate first-order apply kernels
(ddim_apply_kernel / ddim_apply_eps_kernel), so that test_first_order_step_keeps_the_recorded_bits anchors the one merged
kernel outside itself.  Run it again only to add cases, and then only from a tree whose step already passes that test: a file
made from a step that has drifted would record the drift.  x_prev and pred_x0 are stored in full for the small shapes and as
one SHA-256 over both for the clip-sized one.  Needs the GPU:
    python tests/golden/make_ddim_step_bits.py [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ddim_step_bits.npz")
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch

    import test_gpu_multistep as t
    from tooncrafter_amd.ops import HipOps
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the fixture is what the MI355X computes"
    hip, operands, out = HipOps(), t.draw_operands(), {}
    for shape in t.SHAPES:
        for par in ("v", "eps"):
            for guidance, resc, noise in t.BITS_COMBOS:
                x, ec, eu, ei, nz, _ = (t._dev(v) for v in t._case(operands, shape, guidance, noise))
                xp, x0 = hip.ddim_step(x, ec, eu, nz, e_uncond_img=ei, **t._kw(guidance, resc, noise, par))
                assert bool(torch.isfinite(xp).all()) and bool(torch.isfinite(x0).all())
                key = t.bits_key(shape, par, guidance, resc, noise)
                if shape == t.BITS_HASHED:
                    out[key + ".sha256"] = t.bits_digest(xp, x0)
                else:
                    out[key + ".x_prev"], out[key + ".pred_x0"] = xp.cpu().numpy(), x0.cpu().numpy()
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, len(out), "arrays", os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
