#!/usr/bin/env python3
"""Fixture of the relative-position / causal temporal attention (use_relative_position, use_causal_attention of the UNet),
from the REAL reference on the CPU in fp32.  Build container only (needs the reference tree, as make_golden.py does):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_relpos_golden.py

The reference is imported read-only through the stubs of make_golden.py; nothing is copied from it, only parameter names and
tensors that go into and come out of its public UNetModel are saved, to unet_relpos_tiny.npz:

  the reference UNetModel at conftest.TINY_UNET_CFG (temporal_length 4, 8 x 8 latent) on the synthetic weights seed 1234,
  in four variants -- "rel" (use_relative_position), "causal" (use_causal_attention), "both", each on 4 frames, and "rel6":
  relative position on 6 frames, where distances beyond +-4 clamp;
      x4 / ctx4, x6 / ctx6, timesteps, fs        the inputs
      y_rel, y_causal, y_both, y_rel6            the outputs
      y_plain4, y_plain6                         the flagless model on the same inputs
      d_<variant>                                rel-L2 of a variant's output against the flagless one
      table_names, table_values                  every relative_position_{k,v}.embeddings_table and its values
      keys_both                                  the state-dict keys of the "both" model

The synthetic recipe gives a [9, 64] table a standard deviation of 0.07, which moves the output by less than the bound of
the tests, so the tables are drawn here (generator seed 4242, one draw per name in sorted order) and their scale is doubled
until every variant WITH tables is at least MIN_DISTANCE from the flagless output; the causal mask has no scale to raise,
and its distance is asserted as it comes.  A missing term cannot pass the tests.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (install_stubs / the reference's location)
from conftest import TINY_UNET_CFG  # noqa: E402

MIN_DISTANCE = 1e-1
VARIANTS = {"rel": (True, False, 4), "causal": (False, True, 4), "both": (True, True, 4), "rel6": (True, False, 6)}


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm())


def main():
    mg.install_stubs()
    sys.path.insert(0, mg.REF)
    sys.path.insert(1, mg.REPO)
    from tooncrafter_amd import synth                           # noqa: E402  (ours: weight recipe only)
    from lvdm.modules.networks import openaimodel3d as ref_unet  # noqa: E402  (reference)
    assert ref_unet.__file__.startswith(mg.REF)
    torch.manual_seed(0)
    torch.set_grad_enabled(False)

    def build(rel, causal):
        un = ref_unet.UNetModel(**dict(TINY_UNET_CFG, use_relative_position=rel, use_causal_attention=causal)).eval()
        synth.fill_module_(un, prefix="model.diffusion_model.", seed=1234)
        return un

    inputs = {}
    for t in (4, 6):
        inp = synth.synth_inputs(1, t, 8, 8, context_dim=96, seed=11 + t)
        inputs[t] = (torch.cat([inp["x_T"], inp["c_concat"]], dim=1), inp["cond"], inp["fs"])
    ts = torch.tensor([601], dtype=torch.long)
    fwd = lambda m, t: m(inputs[t][0], ts, context=inputs[t][1], fs=inputs[t][2])

    plain = build(False, False)
    y_plain = {t: fwd(plain, t) for t in (4, 6)}
    models = {v: build(rel, causal) for v, (rel, causal, _) in VARIANTS.items()}
    names = sorted(n for n, _ in models["both"].named_parameters() if n.endswith(".embeddings_table"))
    assert names and names == sorted(n for n, _ in models["rel"].named_parameters() if n.endswith(".embeddings_table"))
    assert not [n for n, _ in models["causal"].named_parameters() if n.endswith(".embeddings_table")]
    shapes = {n: tuple(p.shape) for n, p in models["both"].named_parameters() if n in names}
    assert set(shapes.values()) == {(9, 64)}, set(shapes.values())
    g = torch.Generator().manual_seed(4242)
    unit = torch.stack([torch.randn(shapes[n], generator=g) for n in names])

    scale = 0.07
    while True:
        ys, ds = {}, {}
        for v, (rel, _, t) in VARIANTS.items():
            if rel:
                params = dict(models[v].named_parameters())
                for n, u in zip(names, unit):
                    params[n].copy_(u * scale)
            ys[v] = fwd(models[v], t)
            ds[v] = rel_l2(ys[v], y_plain[t])
        print(f"table std {scale:.3f}: distance to the flagless output", {v: f"{d:.3e}" for v, d in ds.items()})
        if all(ds[v] >= MIN_DISTANCE for v, (rel, _, _) in VARIANTS.items() if rel):
            break
        scale *= 2
        assert scale < 50, "the tables do not move the output"
    assert all(d >= MIN_DISTANCE for d in ds.values()), ds
    assert all(torch.isfinite(y).all() for y in ys.values())

    out = dict(x4=inputs[4][0].numpy(), ctx4=inputs[4][1].numpy(), x6=inputs[6][0].numpy(), ctx6=inputs[6][1].numpy(),
               timesteps=ts.numpy(), fs=inputs[4][2].numpy(), y_plain4=y_plain[4].numpy(), y_plain6=y_plain[6].numpy(),
               table_names=np.asarray(names), table_values=(unit * scale).numpy(), table_std=np.float32(scale),
               keys_both=np.asarray(list(models["both"].state_dict().keys())))
    assert torch.equal(inputs[4][2], inputs[6][2])
    for v in VARIANTS:
        out["y_" + v] = ys[v].numpy()
        out["d_" + v] = np.float64(ds[v])
    path = os.path.join(HERE, "unet_relpos_tiny.npz")
    np.savez_compressed(path, **out)
    print("unet_relpos_tiny.npz written:", len(names), "tables,", os.path.getsize(path) // 1024, "KB")


if __name__ == "__main__":
    main()
