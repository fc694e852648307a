"""ctypes loader of libwhisper_hip_ktest.so: the wht_* test entry points over the shipped kernel launchers
(whisper_amd/csrc/ktest.cpp).  Built by `make -C whisper_amd/csrc` (build()) from the same kernel objects as
libwhisper_hip.so.  A missing library is an error: the GPU tests that use it fail, they never skip."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "whisper_amd", "libwhisper_hip_ktest.so")

hipSuccess = 0
hipErrorInvalidValue = 1
hipErrorNotSupported = 801

_P, _I, _L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
SIGNATURES = {
    "wht_last_form": (ctypes.c_char_p, []),
    "wht_clear_form": (None, []),
    "wht_attn_decode_capacity": (_I, [_I]),
    "wht_gemv8_will_run": (_I, [_I, _I, _I, _I]),
    "wht_gemv_family": (ctypes.c_char_p, [_I, _I, _I, _I, _I, _I, _L, _I, _I, _I, _I, _I, _I]),
    "wht_gemv": (_I, [_I, _I, _P, _L, _P, _L, _P, _P, _I, _P, _P, _I, _I, _P, _P, _I, _I, _I, _I, _I, _I, _P, _L, _P, _L,
                      _P, _P, _L, _P, _I, _P, _P, _I, _P, _P]),
    "wht_merge_partials": (_I, [_P, _P, _I, _I, _I, _P, _L, _I, _I, _P]),
    "wht_attn_decode": (_I, [_I, _P, _L, _P, _L, _L, _P, _L, _L, _L, _I, _I, _I, _I, _P, _I, _P, _I, _P, _L, _I, _P, _P, _P,
                             _P, _L, _L, _P]),
    "wht_gemm": (_I, [_I, _I, _I, _P, _L, _L, _P, _L, _L, _P, _L, _L, _P, _I, _P, _L, _L, _I, _I, _I, _I, _I, _P]),
    "wht_attn_flash_f16": (_I, [_P, _L, _L, _P, _L, _L, _P, _L, _L, _P, _L, _L, _I, _I, _I, _I, _I, _P]),
    "wht_layernorm": (_I, [_P, _L, _P, _P, _P, _L, _L, _I, _I, _P]),
    "wht_scatter_kv": (_I, [_P, _I, _I, _I, _P, _I, _P, _P, _I, _P]),
    "wht_gather_cache": (_I, [_P, _P, _P, _I, _L, _L, _P]),
    "wht_permute_groups": (_I, [_P, _P, _I, _L, _I, _I, _L, _L, _P, _P, _L, _P]),
    "wht_replicate_row": (_I, [_P, _L, _I, _L, _I, _I, _I, _L, _P]),
    "wht_xattn_supported": (_I, [_I, _I, _I, _I, _I, _I]),
    "wht_sattn_supported": (_I, [_I, _I, _I, _I]),
    "wht_fused_mode": (_I, [_I]),
    "wht_xattn8": (_I, [_P, _L, _P, _P, _I, _I, _I, _P, _L, _L, _P, _L, _L, _I, _I, _P, _L, _P, _P, _P, _P, _I, _I, _P, _I,
                        _P, _P]),
    "wht_sattn8": (_I, [_P, _L, _P, _P, _I, _I, _I, _P, _P, _L, _P, _P, _P, _P, _L, _P, _P, _I, _I, _P, _I, _P, _P]),
    "wht_beam_kmax": (_I, []),
    "wht_beam_scratch_bytes": (ctypes.c_size_t, [_I, _I]),
    "wht_beam_cand_offsets": (None, [_I, _I, ctypes.POINTER(_L), ctypes.POINTER(_L)]),
    "wht_beam_step": (_I, [_P, _L, _I, _I, _I, _I, _I, _P, _P, _L, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P,
                           ctypes.c_size_t, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "wht_attn_generic": (_I, [_I, _I, _P, _L, _L, _P, _L, _L, _P, _L, _L, _P, _L, _L, _I, _I, _I, _P, _I, _I, _P]),
    "wht_cross_qk": (_I, [_P, _L, _P, _L, _I, _I, _I, _P, _I, _P]),
    "wht_cross_qk_batch": (_I, [_P, _L, _L, _I, _P, _L, _L, _I, _P, _P, _I, _P, _I, _I, _I, _P, _I, _P]),
    "wht_align_batch": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, ctypes.c_float, _P, _I, _P, _P]),
    "wht_dtw": (_I, [_P, _I, _I, _P, _P]),
    "wht_dtw_batch": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _L, _P]),
    "wht_mel_transpose": (_I, [_P, _I, _I, _I, _I, _P, _I, _P]),
    "wht_embed": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _I, _I, _P, _I, _P]),
    "wht_no_speech": (_I, [_P, _L, _I, _I, _I, _P, _P]),
    "wht_gather_rows": (_I, [_P, _P, _I, _I, _P, _P]),
    "wht_gather_tokens": (_I, [_P, _L, _I, _P, _P]),
    # the sampler's noise on the host (sample_noise.h): nothing is launched, no GPU is needed
    "wht_sample_hash": (ctypes.c_uint32, [ctypes.c_uint64, _I, _I, _I]),
    "wht_sample_uniform_of_hash": (ctypes.c_float, [ctypes.c_uint32]),
    "wht_sample_uniform_bits": (_I, []),
    "wht_sample_uniform_range": (None, [ctypes.c_uint32, ctypes.c_uint32, _P]),
    "wht_sample_hash_many": (None, [_P, _P, _P, _P, _L, _P]),
    "wht_rule_mask": (None, [_P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
}

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} missing: build it with `make -C whisper_amd/csrc` (build())")
        h = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(h, name)
            f.restype = res
            f.argtypes = args
        _lib = h
    return _lib


def last_form() -> str:
    return lib().wht_last_form().decode()


def gemv_family(dtype, pro, epi, R, N, K, ld, ln_folded, has_bias, splits, H, frag) -> str:
    """the family launch_gemv picks for the launch _gemv_case (test_kernel_parity_gpu.py) makes of these arguments, asked of
    wht_gemv_family (gemv.hip: pick_family) — nothing is launched; "" = refused.  frag: x_frag where PRO_PLAIN (0), y_frag where
    EPI_STORE (0) / EPI_GELU (3)"""
    return lib().wht_gemv_family(dtype, pro, epi, R, N, K, ld, ln_folded, has_bias, splits, H, int(bool(frag) and pro == 0),
                                 int(bool(frag) and epi in (0, 3))).decode()


def family_of_tag(tag: str) -> str:
    """the family of a gemv form tag (kernels.h: g_form)"""
    if tag.startswith("gemv8/"):
        return "gemv8"
    if tag in ("rows48", "rows48_stream"):
        return tag
    if tag.startswith("rows16_mf<"):
        return "rows16_mf"
    for head in ("rt<", "stream<"):
        if tag.startswith(head):
            rt = tag[len(head):tag.index(">")].split(",")[1]
            assert rt in ("4", "8"), tag
            return "rt" + rt
    raise AssertionError(f"not a gemv form tag: {tag!r}")
