"""CPU check of the SHIPPED gfx950 code object: the cached-prefill kernel (`attn_prefill_kernel`, every instance of the contiguous
and of the paged cache) is there, uses the int8 score MFMA and the transposed V reads, and keeps its loops free of scratch
traffic; and adding it left the decode and dense families as they were.  Same analysis as tests/test_decode_codeobj_cpu.py."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_mfma_hazards as chk  # noqa: E402


@pytest.fixture(scope="module")
def fns():
    so = os.path.join(ROOT, "lowbit_quant_fa2_paddle_amd", "liblowbit_fa_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    return chk.parse(chk.disassemble(so))


@pytest.mark.skipif(not chk.tools_available(), reason="llvm-objdump / clang-offload-bundler not found under /opt/rocm")
@pytest.mark.parametrize("kv", ["ContiguousKV", "PagedKV"], ids=["contiguous", "paged"])
def test_prefill_instances_and_their_loops(fns, kv):
    prefill = {name: ins for name, ins in fns.items() if "attn_prefill_kernel" in name and kv in name}
    assert len(prefill) == 4, sorted(prefill)  # 2 dtypes x 2 head dims
    assert sum("attn_prefill_kernel" in name for name in fns) == 8  # and no instance outside the two layouts
    for name, ins in prefill.items():
        assert any(mn == "v_mfma_i32_16x16x64_i8" for _, mn, _, _ in ins), name     # the int8 score product ...
        assert any(mn == "v_mfma_f32_16x16x32_f16" for _, mn, _, _ in ins), name    # ... the fp16 P V product ...
        assert any(mn == "ds_read_b64_tr_b16" for _, mn, _, _ in ins), name          # ... and the transposed V reads are there
    over = {name: n for name, ins in prefill.items() if (n := chk.scratch_in_loops(ins))}
    assert not over, over
    # the new kernel is in neither family the other static checks count
    assert not any("attn_decode_kernel" in name or "attn_fwd" in name for name in prefill)
    assert sum("attn_decode_kernel" in name for name in fns) == 24
