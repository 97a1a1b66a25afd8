"""Shared by tests/test_torch_ops_cpu.py and tests/test_gpu_torch_ops.py: one malformed request per operator family of
`torch.ops.tooncrafter` (csrc/torch_ops.cpp), with the smallest tensors that reach the check.  Every operator is one function
under the CUDA and the Meta key, so each request is refused on either device, in the same words, before anything is launched."""
import torch


def malformed_requests(device):
    """family -> (operator name, arguments) on `device`.  torch.empty only: building the requests runs no kernel."""
    def e(*shape, dtype=torch.bfloat16):
        return torch.empty(*shape, dtype=dtype, device=device)

    f32, u8 = torch.float32, torch.uint8
    lat = e(1, 4, 2, 2, 2, dtype=f32)
    other = e(1, 4, 2, 2, 3, dtype=f32)
    g = e(64, dtype=f32)
    return {
        # bias of the wrong length
        "gemm": ("gemm", (e(8, 64), e(64, 64), e(63, dtype=f32), None, None, 0, 0, 1.0, 1.0, False, [])),
        # K rows not kv_batches * lk (2 * 3)
        "attention": ("attention", (e(2 * 4, 64), e(7, 64), e(7, 64), 2, 1, 4, 3, 1, 0.125, None, None, 0, 1)),
        # V rows wrong
        "attention_q8": ("attention_q8", (e(2 * 4, 64), e(2 * 4, 64), e(7, 64), 2, 1, 4, 4, 0.125)),
        # x rows not samples * rows (2 * 8)
        "groupnorm": ("groupnorm", (e(2 * 7, 64), g, g, 2, 8, 1e-5, False)),
        # five prefetch tensors (TC_PREFETCH_MAX is 4)
        "layernorm_pf": ("layernorm_pf", (e(8, 64), g, g, 1e-5, [e(8) for _ in range(5)])),
        # x0_hist of another shape
        "ddim_step_ms": ("ddim_step_ms", (lat, lat, None, None, None, other, 0.25, 1.0, 1.0, 0.0, 0.6, 0.8, 0.7, 0.5, 0.0, 1.0)),
        # mask of another shape
        "ddim_blend": ("ddim_blend", (lat, lat, None, other, 0.6, 0.8)),
        # c = 128 with one head
        "temporal_qkv_attn": ("temporal_qkv_attn", (e(1 * 2 * 4, 128), e(384, 128), None, 1, 2, 4, 1, 0.125)),
        # slot 2 of a clip tensor with 1 * 2 frames
        "frames_from_u8": ("frames_from_u8", (e(1, 8, 8, 3, dtype=u8), [2], 1, 2, 8, 8, None, None, None, None)),
        # an odd height for I420
        "frames_to_u8": ("frames_to_u8", (e(1, 3, 2, 8, 8, dtype=f32), 7, 8, 1, 0, 2, None, None, None, None)),
        # k not a multiple of 32
        "quant_mxfp8": ("quant_mxfp8", (e(8, 64), 48)),
    }


FAMILIES = tuple(malformed_requests("meta"))
