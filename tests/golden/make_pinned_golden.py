#!/usr/bin/env python3
"""Golden trajectories of pinned-frame (mask / x0) and partial (timesteps=, stochastic_encode, decode) DDIM runs, from
the REAL reference on the tiny model.  Build container only (needs the reference tree, as make_golden.py does):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_pinned_golden.py [--out FILE]    # -> ddim_pinned_tiny.npz

The reference is imported read-only through the stubs and the tiny configuration of make_golden.py; nothing is copied
from it, only tensors that go into and come out of its public classes are saved.  Settings of ddim_tiny.npz: T, H, W =
4, 8, 8; S = 5, eta 1, uniform_trailing, CFG 7.5, guidance rescale 0.7; the inputs of synth.synth_inputs(seed=7).

Runs (prefix of the arrays of each):
  a_  DDIMSampler, mask (1,1,4,1,1) with frame 2 = 1
  b_  the same with clean_cond=True (x0 blended in un-noised; no q_sample draw)
  c_  DDIMSampler, dense random 0/1 mask (1,4,4,8,8)
  d_  the three-way sampler (ddim_multiplecond.py) with a_'s mask and cfg_img = 3.0
  e_  timesteps=3 from x_T = stochastic_encode(x0, t=[1], noise=e_enc_noise); e_x_T is that encoding
  f_  decode(e_x_T, t_start=2) at CFG 7.5 (the reference hands it neither fs nor a guidance rescale)
Per run: `noises` (the noise_like draws, in order), `qnoises` (the q_sample draws, in order), `pred_x0` per step,
`samples`, `t` (the timesteps at which the UNet ran).  Shared: x0, mask_frame, mask_dense, the conditioning, x_T, and
subset_t_<k>: the timesteps a `timesteps=k` run walks, for k in 1, 3, 5, 9.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (install_stubs / tiny_config / the reference's location)

S, T, H, W = 5, 4, 8, 8
SETTINGS = dict(unconditional_guidance_scale=7.5, eta=1.0, timestep_spacing="uniform_trailing", guidance_rescale=0.7)


def main(out_path):
    mg.install_stubs()
    sys.path.insert(0, mg.REF)
    sys.path.insert(1, mg.REPO)
    from tooncrafter_amd import synth                        # noqa: E402  (ours: weight recipe only)
    from utils.utils import instantiate_from_config          # noqa: E402  (reference)
    from lvdm.models.samplers import ddim as ref_ddim        # noqa: E402
    from lvdm.models.samplers import ddim_multiplecond as ref_mc   # noqa: E402
    assert ref_ddim.__file__.startswith(mg.REF) and ref_mc.__file__.startswith(mg.REF)
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    for mod in (ref_ddim, ref_mc):                           # CPU (ddim.py:18-22 hard-codes cuda)
        mod.DDIMSampler.register_buffer = lambda self, n, a: setattr(self, n, a)
    model = instantiate_from_config(mg.tiny_config().model).eval()
    model.perframe_ae = True
    synth.fill_module_(model, seed=1234)

    inp = synth.synth_inputs(1, T, H, W, context_dim=96, seed=7)
    cond = {"c_crossattn": [inp["cond"]], "c_concat": [inp["c_concat"]]}
    uc = {"c_crossattn": [inp["uncond"]], "c_concat": [inp["c_concat"]]}
    uc_img_ctx = torch.cat([inp["uncond"][:, :77], inp["cond"][:, 77:]], dim=1)      # text dropped, image tokens kept
    uc_img = {"c_crossattn": [uc_img_ctx], "c_concat": [inp["c_concat"]]}
    shape = tuple(inp["x_T"].shape)
    g = torch.Generator().manual_seed(4242)
    x0 = torch.randn(shape, generator=g)
    mask_frame = torch.zeros(1, 1, T, 1, 1)
    mask_frame[:, :, 2] = 1.0
    mask_dense = (torch.rand(shape, generator=g) < 0.5).to(torch.float32)
    out = dict(x0=x0.numpy(), mask_frame=mask_frame.numpy(), mask_dense=mask_dense.numpy(), x_T=inp["x_T"].numpy(),
               c_concat=inp["c_concat"].numpy(), cond=inp["cond"].numpy(), uncond=inp["uncond"].numpy(),
               uncond_img=uc_img_ctx.numpy(), fs=inp["fs"].numpy(), cfg_img=np.float32(3.0))

    orig_apply, orig_q = model.apply_model, model.q_sample

    def record(tag, mod, call):
        """Run `call(sampler, pred_x0 sink)` with every random draw injected and recorded."""
        noises = [torch.randn(shape, generator=g) for _ in range(S)]
        qnoises = [torch.randn(shape, generator=g) for _ in range(S)]
        it, qit, used, qused, ts, x0s = iter(noises), iter(qnoises), [], [], [], []

        def noise_like(shp, device, repeat=False):
            used.append(next(it))
            return used[-1]

        def q_sample(x_start, t, noise=None):
            qused.append(next(qit))
            return orig_q(x_start, t, noise=qused[-1])

        def apply_model(x, t, c, **kw):
            if not ts or ts[-1] != int(t[0]):
                ts.append(int(t[0]))
            return orig_apply(x, t, c, **kw)

        mod.noise_like, model.q_sample, model.apply_model = noise_like, q_sample, apply_model
        try:
            samples = call(mod.DDIMSampler(model), x0s)
        finally:
            model.q_sample, model.apply_model = orig_q, orig_apply
        stack = lambda lst: torch.stack(lst).numpy() if lst else np.zeros((0, *shape), dtype=np.float32)
        out.update({tag + "noises": stack(used), tag + "qnoises": stack(qused), tag + "pred_x0": stack(x0s),
                    tag + "samples": samples.numpy(), tag + "t": np.asarray(ts, dtype=np.int64)})
        print(f"{tag} t {ts}  q draws {len(qused)}  final std {float(samples.std()):.4f}  "
              f"finite {bool(torch.isfinite(samples).all())}", flush=True)
        return samples

    def sample(sampler, x0s, *, x_T=inp["x_T"], **kw):
        res, _ = sampler.sample(S=S, conditioning=cond, batch_size=1, shape=shape[1:], verbose=False,
                                unconditional_conditioning=uc, fs=inp["fs"], x_T=x_T,
                                img_callback=lambda p, i: x0s.append(p.clone()), **SETTINGS, **kw)
        return res

    three_way = dict(cfg_img=3.0, unconditional_conditioning_img_nonetext=uc_img)
    record("a_", ref_ddim, lambda s, sink: sample(s, sink, mask=mask_frame, x0=x0))
    record("b_", ref_ddim, lambda s, sink: sample(s, sink, mask=mask_frame, x0=x0, clean_cond=True))
    record("c_", ref_ddim, lambda s, sink: sample(s, sink, mask=mask_dense, x0=x0))
    record("d_", ref_mc, lambda s, sink: sample(s, sink, mask=mask_frame, x0=x0, **three_way))

    enc_noise = torch.randn(shape, generator=g)
    enc = ref_ddim.DDIMSampler(model)
    enc.make_schedule(S, ddim_discretize="uniform_trailing", ddim_eta=1.0, verbose=False)
    e_x_T = enc.stochastic_encode(x0, torch.tensor([1]), noise=enc_noise)
    out.update(e_enc_noise=enc_noise.numpy(), e_x_T=e_x_T.numpy())
    record("e_", ref_ddim, lambda s, sink: sample(s, sink, x_T=e_x_T, timesteps=3))

    def decode(sampler, x0s):
        sampler.make_schedule(S, ddim_discretize="uniform_trailing", ddim_eta=1.0, verbose=False)
        step = sampler.p_sample_ddim

        def p_sample_ddim(*a, **kw):                        # decode() drops pred_x0: keep it for the fixture
            res = step(*a, **kw)
            x0s.append(res[1].clone())
            return res
        sampler.p_sample_ddim = p_sample_ddim
        return sampler.decode(e_x_T, cond, 2, unconditional_guidance_scale=7.5, unconditional_conditioning=uc)
    record("f_", ref_ddim, decode)

    for k in (1, 3, 5, 9):                                   # which steps a partial run walks (ddim.py:152-156)
        tag = f"sub{k}_"
        record(tag, ref_ddim, lambda s, sink: sample(s, sink, timesteps=k))
        out[f"subset_t_{k}"] = out[tag + "t"]
        for key in [key for key in out if key.startswith(tag)]:
            del out[key]

    np.savez_compressed(out_path, **out)
    print(f"{out_path} written ({os.path.getsize(out_path) / 1024:.0f} KB)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "ddim_pinned_tiny.npz"))
    main(ap.parse_args().out)
