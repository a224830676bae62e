"""CPU check of the SHIPPED gfx950 code object: the decode attention kernel (`attn_decode_kernel`, every instance of the
contiguous and of the paged cache) is there, uses the int8 score MFMA and the transposed V reads, and keeps its tile loop free
of scratch traffic.  The kernel is HBM-bound: a spill in the loop - the paged table look-up must not cost one either - adds
memory traffic to the very resource that limits it.  Same analysis as tests/test_hazards_cpu.py uses for the prefill kernels
(tools/check_mfma_hazards.py).  The instances are told apart by the policy in their names (attn_decode.hip, kvcache.hip)."""
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
@pytest.mark.parametrize("kv, dst", [("ContiguousKV", "ContiguousDst"), ("PagedKV", "PagedDst")], ids=["contiguous", "paged"])
def test_decode_tile_loop_has_no_scratch_traffic(fns, kv, dst):
    decode = {name: ins for name, ins in fns.items() if "attn_decode_kernel" in name and kv in name}
    # 2 dtypes x 2 head dims x 3 row-block counts
    assert len(decode) == 12, sorted(decode)
    assert sum("attn_decode_kernel" in name for name in fns) == 24  # and no instance outside the two layouts
    for name, ins in decode.items():
        assert any(mn == "v_mfma_i32_16x16x64_i8" for _, mn, _, _ in ins), name     # the int8 score product ...
        assert any(mn == "ds_read_b64_tr_b16" for _, mn, _, _ in ins), name          # ... and the transposed V reads are there
    over = {name: n for name, ins in decode.items() if (n := chk.scratch_in_loops(ins))}
    assert not over, over
    assert sum("kvcache_append_kernel" in name and dst in name for name in fns) == 4  # 2 dtypes x 2 head dims
