"""lowbit_quant_fa2_paddle_amd - MI355X-native low-bit FlashAttention-2 forward.

Same public names as the reference package (src/__init__.py:1-17).
"""
from .core import (  # noqa: F401
    # Legacy names (backward-compatible)
    sageattn,
    sageattn_varlen,
    sageattn_qk_int8_pv_fp16_triton,
    sageattn_qk_int8_pv_fp16_cuda,
    sageattn_qk_int8_pv_fp8_cuda,
    sageattn_qk_int4_pv_fp16_triton,
    sageattn_multi_precision,
    # Preferred new names
    lowbit_fa_attn,
    lowbit_fa_varlen,
    lowbit_fa_multi_precision,
    lowbit_fa_qk_int8_pv_fp16_triton,
    lowbit_fa_qk_int8_pv_fp16_cuda,
    lowbit_fa_qk_int8_pv_fp8_cuda,
    lowbit_fa_qk_int4_pv_fp16_triton,
)
from .kvcache import (  # noqa: F401
    # int8 KV cache + split-KV decode attention (no counterpart that works in the reference: SURVEY.md row 8)
    LowbitKVCache,
    LowbitPagedKVCache,
    PageAllocator,
    lowbit_fa_decode,
    sageattn_decode,
    # cached prefill: any number of queries over the same caches
    lowbit_fa_prefill,
    sageattn_prefill,
)

__version__ = "0.1.0"
