"""CPU check of the SHIPPED gfx950 code object: the paged decode attention kernel (`attn_paged_decode_kernel`, every instance)
is there, uses the int8 score MFMA and the transposed V reads of the contiguous kernel, and keeps its tile loop free of scratch
traffic - the table look-up must not cost the HBM-bound loop a spill.  Same analysis as tests/test_decode_codeobj_cpu.py."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_mfma_hazards as chk  # noqa: E402


@pytest.mark.skipif(not chk.tools_available(), reason="llvm-objdump / clang-offload-bundler not found under /opt/rocm")
def test_paged_decode_tile_loop_has_no_scratch_traffic():
    so = os.path.join(ROOT, "lowbit_quant_fa2_paddle_amd", "liblowbit_fa_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    fns = chk.parse(chk.disassemble(so))
    paged = {name: ins for name, ins in fns.items() if "attn_paged_decode_kernel" in name}
    # 2 dtypes x 2 head dims x 3 row-block counts
    assert len(paged) == 12, sorted(paged)
    assert not any("attn_decode_kernel" in name for name in paged)  # the contiguous kernel's count stays 12
    for name, ins in paged.items():
        assert any(mn == "v_mfma_i32_16x16x64_i8" for _, mn, _, _ in ins), name
        assert any(mn == "ds_read_b64_tr_b16" for _, mn, _, _ in ins), name
    over = {name: n for name, ins in paged.items() if (n := chk.scratch_in_loops(ins))}
    assert not over, over
    assert sum("kvcache_paged_append_kernel" in name for name in fns) == 4  # 2 dtypes x 2 head dims
