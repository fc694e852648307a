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
