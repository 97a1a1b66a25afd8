"""Long-clip (T = 32) full-size UNet parity case shared by the golden generator (tests/golden/make_long_clip_golden.py,
runs the fp32 CPU oracle) and the GPU test (tests/test_gpu_long_clip.py, runs the HIP path).

The reference's inference.py takes --video_length N for any N; at N != 16 its image projection still yields 16 x 16
tokens, so the context is 77 + 256 long, not 77 + 16 N, and openaimodel3d.py:556-562 gives every frame the same
image tokens.  That is the case pinned here: T = 32 frames at the 40 x 64 latent of 320 x 512 pixels, weights and
inputs from seeds only.  The output (1.3 MB in fp32) is kept at sampled positions plus its norm.
"""
import os

import torch

from conftest import FULL_UNET_CFG, GOLDEN
from fullsize_cases import full_state_dict, sample_idx  # noqa: F401  (re-exported for the golden generator)
from tooncrafter_amd import synth

GOLDEN_FILE = os.path.join(GOLDEN, "long_clip_oracle.npz")
T, H, W = 32, 40, 64
UNET_T = 601
N_OUT = 65536
UNET_CFG = dict(FULL_UNET_CFG, temporal_length=T)


def inputs():
    """x_T, c_concat, a context of 77 text + 256 shared image tokens, fs."""
    inp = synth.synth_inputs(1, T, H, W, n_img_tokens_per_frame=8, seed=11)       # 77 + 8 * 32 = 77 + 256
    assert inp["cond"].shape[1] == 77 + 256
    return inp
