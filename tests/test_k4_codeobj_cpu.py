"""CPU check of the SHIPPED gfx950 code object: the packed-K families (`attn_decode_k4_kernel`, `attn_decode_k4_v8_kernel`,
`attn_prefill_k4_kernel`, `attn_prefill_k4_v8_kernel`, `kvcache_append_k4_kernel`, `kvcache_append_k4_v8_kernel`) are there with
the instance counts of their byte-per-code siblings, each reader uses the int8 score MFMA, the fp16 P V MFMA and the transposed V
reads - the nibbles are widened in front of the score product, everything behind it is the sibling's kernel - and keeps its loops
free of scratch traffic.  Same analysis as tests/test_v8_codeobj_cpu.py."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_mfma_hazards as chk  # noqa: E402

OLD_FAMILIES = ("attn_decode_kernel", "attn_decode_v8_kernel", "attn_prefill_kernel", "attn_prefill_v8_kernel", "kvcache_append_kernel",
                "kvcache_append_v8_kernel", "attn_fwd")


@pytest.fixture(scope="module")
def fns():
    so = os.path.join(ROOT, "lowbit_quant_fa2_paddle_amd", "liblowbit_fa_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    return chk.parse(chk.disassemble(so))


@pytest.mark.skipif(not chk.tools_available(), reason="llvm-objdump / clang-offload-bundler not found under /opt/rocm")
@pytest.mark.parametrize("kv, dst", [("ContiguousKV", "ContiguousDst"), ("PagedKV", "PagedDst")], ids=["contiguous", "paged"])
def test_k4_families(fns, kv, dst):
    # 2 dtypes x 2 head dims (x 3 row-block counts), fp16 V and fp8 V: the counts of the byte-per-code families
    readers = {}
    for family, count in (("attn_decode_k4_kernel", 12), ("attn_decode_k4_v8_kernel", 12), ("attn_prefill_k4_kernel", 4),
                          ("attn_prefill_k4_v8_kernel", 4)):
        got = {name: ins for name, ins in fns.items() if family in name and kv in name}
        assert len(got) == count, (family, sorted(got))
        assert sum(family in name for name in fns) == 2 * count, family  # and no instance outside the two layouts
        readers.update(got)
    assert len(readers) == 32
    for name, ins in readers.items():
        for mn in ("v_mfma_i32_16x16x64_i8", "v_mfma_f32_16x16x32_f16", "ds_read_b64_tr_b16"):
            assert any(m == mn for _, m, _, _ in ins), (name, mn)
    over = {name: n for name, ins in readers.items() if (n := chk.scratch_in_loops(ins))}
    assert not over, over
    for family in ("kvcache_append_k4_kernel", "kvcache_append_k4_v8_kernel"):
        assert sum(family in name and dst in name for name in fns) == 4, family
        assert sum(family in name for name in fns) == 8, family
    # the new families are in none of the families the other static checks count
    new = [name for name in fns if "_k4_" in name]
    assert len(new) == 80
    assert not any(k in name for name in new for k in OLD_FAMILIES)
