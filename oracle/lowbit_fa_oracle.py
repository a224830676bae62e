"""CPU oracle for the low-bit FlashAttention-2 forward hot path.

TEST INFRASTRUCTURE ONLY.  Nothing under ``lowbit_quant_fa2_paddle_amd/`` may import this
module: it is the *checker* used by ``tests/``, ``__graft_entry__.smoke()`` and the
``cpu_baseline`` leg of ``bench.py``; the product path is the HIP library and fails loudly
when that library is missing.

What this file is: a numpy restatement of the reference's algorithm for the path
``lowbit_fa_qk_int{8,4}_pv_fp{16,8}_*`` (reference = Charles2530/lowbit_quant_fa2_paddle,
paths below are relative to that tree).  Every function cites the reference lines it
follows.  It is written for clarity and bit-level faithfulness, not speed; rows are
independent in the tile loop, so the loop over 64-key tiles is kept sequential (the online
softmax order matters) and everything else is vectorised over rows.

Parity pin: the int8 / fp16 functions are pinned against golden vectors produced by the
reference's own ``@triton.jit`` kernels executed under ``TRITON_INTERPRET=1`` (see
``tests/golden/make_golden.py`` and ``tests/test_oracle_golden.py``).  The fp8-PV functions
restate CUDA code that cannot be executed here (``csrc/qattn/qk_int_sv_f8_cuda.cu``) and
the reference holds no fixture for them: **parity unpinned** for fp8-PV, checked only
against fp32 SDPA within a stated tolerance.
"""
from __future__ import annotations

import math

import numpy as np

LOG2E = 1.44269504  # the literal the reference uses (src/triton/quant_per_block.py:226, src/core.py:347)
FP8_E4M3_MAX = 448.0
FP8_P_OFFSET = 8.807  # csrc/qattn/attn_utils.cuh:30  (log2(448) rounded) -> P_max = 448


# --------------------------------------------------------------------------------------
# dtype helpers
# --------------------------------------------------------------------------------------
def bf16_round(x: np.ndarray) -> np.ndarray:
    """Round fp32 -> bf16 (RNE) and return the value as fp32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    out = (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(x), x, out)


def to_storage(x: np.ndarray, dtype: str) -> np.ndarray:
    """Round an fp32 array to the value set of `dtype` ('fp16'|'bf16'), returned as fp32."""
    if dtype == "fp16":
        return x.astype(np.float16).astype(np.float32)
    if dtype == "bf16":
        return bf16_round(x)
    raise ValueError(dtype)


def e4m3fn_round(x: np.ndarray) -> np.ndarray:
    """fp32 -> OCP e4m3fn, round-to-nearest-even, saturate-to-finite (+-448); value as fp32.

    Follows the conversion the reference uses (`cvt.rn.satfinite.e4m3x2.f32`,
    csrc/numeric_conversion.cuh:39-54).  e4m3fn: 4 exponent bits (bias 7), 3 mantissa bits,
    min normal 2^-6, subnormal step 2^-9, max 448.
    """
    x = np.asarray(x, dtype=np.float32)
    a = np.abs(x).astype(np.float64)
    a = np.minimum(a, FP8_E4M3_MAX)
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -20)))
    e = np.maximum(e, -6.0)  # subnormals share the exponent of the smallest normal
    step = 2.0 ** (e - 3)
    q = np.rint(a / step) * step  # np.rint = round-half-even
    q = np.minimum(q, FP8_E4M3_MAX)
    return np.copysign(q, x).astype(np.float32)  # keeps the sign of a zero, as the hardware conversions do


def e4m3fn_encode(x: np.ndarray) -> np.ndarray:
    """Values already on the e4m3fn grid -> uint8 bit patterns."""
    x = np.asarray(x, dtype=np.float32)
    s = (np.signbit(x)).astype(np.uint8) << 7
    a = np.abs(x).astype(np.float64)
    out = np.zeros(a.shape, dtype=np.uint8)
    nz = a > 0
    e = np.floor(np.log2(np.where(nz, a, 1.0)))
    e = np.maximum(e, -6.0)
    is_sub = a < 2.0 ** -6
    mant = np.where(is_sub, a / 2.0 ** -9, (a / 2.0 ** e - 1.0) * 8.0)
    ebits = np.where(is_sub, 0, e + 7).astype(np.int64)
    out = (ebits.astype(np.uint8) << 3) | np.rint(mant).astype(np.uint8)
    out = np.where(nz, out, 0).astype(np.uint8)
    return out | s


def e4m3fn_decode(b: np.ndarray) -> np.ndarray:
    b = np.asarray(b, dtype=np.uint8)
    s = np.where(b & 0x80, -1.0, 1.0)
    e = ((b >> 3) & 0xF).astype(np.int64)
    m = (b & 0x7).astype(np.float64)
    v = np.where(e == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * 2.0 ** (e - 7.0))
    return (s * v).astype(np.float32)


# --------------------------------------------------------------------------------------
# L2: per-block quantisation  (src/triton/quant_per_block.py)
# --------------------------------------------------------------------------------------
def quant_per_block(x: np.ndarray, sm_scale: float, qmax: float, blk: int, amax_floor: float = 0.0):
    """One tensor, canonical [B, H, S, C] fp32 values (already rounded to the storage dtype).

    Restates `quant_per_block_int8_kernel` (src/triton/quant_per_block.py:132-178, qmax=127)
    and `quant_per_block_int4_unpack_kernel` (:22-71, qmax=7):
        x = load(masked rows -> 0).to(fp32); x *= sm_scale; scale = max|x| / qmax;
        y = x / scale; y += 0.5*sign(y) (sign(0) := +1); int8(trunc(y)); one scale per block.
    `amax_floor`: the reference has no epsilon (:173) so an all-zero block yields scale=0 and
    NaN codes; the CUDA quantiser floors amax at 1e-7 (csrc/fused/fused.cu:147).  The HIP path
    adopts the floor; with the floor the result is bit-identical whenever amax >= 1e-7.
    Returns (codes int8 [B,H,S,C], scale fp32 [B,H,ceil(S/blk)]).
    """
    B, H, S, C = x.shape
    nblk = (S + blk - 1) // blk
    pad = nblk * blk - S
    xf = x.astype(np.float32)
    if pad:
        xf = np.concatenate([xf, np.zeros((B, H, pad, C), np.float32)], axis=2)
    xf = xf * np.float32(sm_scale)
    xb = xf.reshape(B, H, nblk, blk * C)
    amax = np.max(np.abs(xb), axis=-1)
    if amax_floor > 0.0:
        amax = np.maximum(amax, np.float32(amax_floor))
    scale = (amax / np.float32(qmax)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        y = xb / scale[..., None]
        y = y + np.float32(0.5) * np.where(y >= 0, np.float32(1), np.float32(-1))
        y = np.nan_to_num(y, nan=0.0)
    codes = np.trunc(y).astype(np.int32).astype(np.int8)
    codes = codes.reshape(B, H, nblk * blk, C)[:, :, :S]
    return np.ascontiguousarray(codes), scale


def mean_seq(k: np.ndarray, dtype: str) -> np.ndarray:
    """`km = k.mean(dim=seq, keepdim=True)` (src/core.py:292-293): fp32 accumulate, result
    rounded to the storage dtype.  k canonical [B,H,S,D] fp32-valued.  Returns [B,H,1,D]."""
    m = np.mean(k.astype(np.float64), axis=2, keepdims=True).astype(np.float32)
    return to_storage(m, dtype)


def per_block_int8(q, k, km, sm_scale, dtype: str, BLKQ=128, BLKK=64, q_qmax=127.0, k_qmax=127.0,
                   amax_floor: float = 0.0):
    """Host wrapper `per_block_int8` (src/triton/quant_per_block.py:181-248); with
    q_qmax=k_qmax=7 it is `per_block_int4_unpack` (:251-318); q_qmax=127,k_qmax=7 is the
    intent of `per_block_q_int8_k_int4` (:391-458, defective as written - SURVEY 2.4-5).

    `k - km` is an elementwise op in the storage dtype (:186-187) -> rounded to that dtype.
    Q gets sm_scale*1.44269504 folded in (:226), K uses 1.0 (:244).
    Canonical [B,H,S,D] arrays in / out.
    """
    if km is not None:
        k = to_storage(k.astype(np.float32) - km.astype(np.float32), dtype)
    # the product is formed in Python double and reaches the kernel as ONE fp32 argument (:226)
    q_i8, q_scale = quant_per_block(q, np.float32(float(sm_scale) * LOG2E), q_qmax, BLKQ, amax_floor)
    k_i8, k_scale = quant_per_block(k, 1.0, k_qmax, BLKK, amax_floor)
    return q_i8, q_scale, k_i8, k_scale


# --------------------------------------------------------------------------------------
# chosen Q blocks of a long sequence
# --------------------------------------------------------------------------------------
def block_rows(q_blocks, S: int, BLOCK_M: int = 128) -> np.ndarray:
    """Absolute row indices of the Q blocks `q_blocks` (ascending block indices) of a sequence of S rows, in order: what a
    caller slices out of Q (or of a device output) to hand the oracle's `q_blocks` paths."""
    blocks = [int(b) for b in q_blocks]
    assert blocks == sorted(set(blocks)) and blocks and 0 <= blocks[0] and blocks[-1] * BLOCK_M < S, (blocks, S)
    return np.concatenate([np.arange(b * BLOCK_M, min((b + 1) * BLOCK_M, S)) for b in blocks])


def _rows_of_blocks(q_blocks, n_rows: int, BLOCK_M: int = 128) -> np.ndarray:
    """Absolute row indices of `n_rows` given rows that hold the Q blocks `q_blocks` back to back: whole blocks, only the last
    one may be short (the ragged last block of the sequence).  None -> rows 0 .. n_rows - 1."""
    if q_blocks is None:
        return np.arange(n_rows)
    blocks = [int(b) for b in q_blocks]
    assert blocks == sorted(set(blocks)) and blocks and blocks[0] >= 0, blocks
    last = n_rows - BLOCK_M * (len(blocks) - 1)
    assert 0 < last <= BLOCK_M, f"{n_rows} rows cannot hold the blocks {blocks} (whole blocks, the last one may be short)"
    return np.concatenate([np.arange(b * BLOCK_M, b * BLOCK_M + (BLOCK_M if i + 1 < len(blocks) else last))
                           for i, b in enumerate(blocks)])


def _split_by_direction(q_blocks, n_blocks: int, key_tiles_reversed):
    """Per-block key-tile order: `key_tiles_reversed` is one bool for the call or one per given Q block.  -> None when every
    block walks the same way, else the two lists of given-block positions (forward, reversed)."""
    if isinstance(key_tiles_reversed, (bool, np.bool_)):
        return None
    rev = [bool(r) for r in key_tiles_reversed]
    assert len(rev) == n_blocks, f"key_tiles_reversed: {len(rev)} flags for {n_blocks} Q blocks"
    if all(rev) or not any(rev):
        return None
    return [i for i, r in enumerate(rev) if not r], [i for i, r in enumerate(rev) if r]


def _by_direction(fn, split, q_blocks, Sq: int, BLOCK_M: int, row_args: dict, blk_args: dict, kw: dict, n_out: int):
    """Run `fn` once per key-tile direction on the given Q blocks that walk that way (rows are independent) and put the
    row-shaped results back in place.  row_args: arrays with the given rows on axis 2; blk_args: arrays with one entry per
    given block on axis 2."""
    nb = (Sq + BLOCK_M - 1) // BLOCK_M
    blocks = list(range(nb)) if q_blocks is None else [int(b) for b in q_blocks]
    outs = None
    for pos, rev in zip(split, (False, True)):
        lr = np.concatenate([np.arange(i * BLOCK_M, min((i + 1) * BLOCK_M, Sq)) for i in pos])
        res = fn(**{k: a[:, :, lr] for k, a in row_args.items()}, **{k: a[:, :, pos] for k, a in blk_args.items()}, **kw,
                 q_blocks=[blocks[i] for i in pos], key_tiles_reversed=rev)
        res = res if isinstance(res, tuple) else (res,)
        if outs is None:
            outs = [None if r is None else np.zeros(r.shape[:2] + (Sq,) + r.shape[3:], r.dtype) for r in res[:n_out]]
        for o, r in zip(outs, res):
            if o is not None:
                o[:, :, lr] = r
    return tuple(outs)


# --------------------------------------------------------------------------------------
# L1: fused attention tile loop  (src/triton/attn_qk_int8_per_block{,_causal}.py)
# --------------------------------------------------------------------------------------
def attn_fwd_int8_fp16(q_i8, k_i8, v16, q_scale, k_scale, *, causal: bool, out_dtype: str = "fp16",
                       return_lse: bool = False, BLOCK_M: int = 128, BLOCK_N: int = 64,
                       tail: str = "reference", pv_tile_fp16: bool = True, causal_mask: str = "reference", q_blocks=None):
    """`_attn_fwd` + `_attn_fwd_inner` (src/triton/attn_qk_int8_per_block.py:69-167 / :24-66) and the
    causal pair (src/triton/attn_qk_int8_per_block_causal.py:82-214 / :24-79).

    q_i8 [B,Hq,Sq,D] int8, k_i8 [B,Hkv,Sk,D] int8, v16 [B,Hkv,Sk,D] (fp16 values),
    q_scale [B,Hq,ceil(Sq/128)], k_scale [B,Hkv,ceil(Sk/64)] fp32.
    Per 64-key tile:  qk = int32(q.k) -> fp32 * q_scale * k_scale (:51);  m_ij = max(m_i, rowmax);
    p = exp2(qk - m_ij); l = l*alpha + sum(p); acc *= alpha (:52-58);  acc += fp16(dot(p.fp16, v))
    (:59-61, tile product rounded to fp16 when `pv_tile_fp16`, the reference's out_dtype=fp16);
    epilogue acc * (1/l) (:161-162), lse = log2(l) + m (:164-167, base-2 domain).
    Causal: tiles below the diagonal block unmasked (STAGE 1, causal :45-46), the 128x128 diagonal
    block gets `qk += where(row >= col, 0, -1e6)` (STAGE 2, :47-63); tiles above are never visited.
    `tail`: 'reference' = out-of-range K columns load as 0 so qk=0 takes part in the softmax
    (:48-49, the reference's ragged-tail defect); 'neg_inf' = masked with -inf (what
    the CUDA path does, csrc/qattn/attn_utils.cuh:327-353, and what the HIP kernel does).
    `causal_mask`: 'reference' = the additive -1e6 of STAGE 2 (a key above the diagonal still takes part once scores reach
    ~1e6 binades, q, k of ~1000 N(0,1)); 'neg_inf' = masked with -inf, as the HIP kernels and the CUDA path do.  The two agree
    bit for bit while every score is far below 1e6 binades.
    `q_blocks` (ascending block indices): the given Q rows are those 128-row blocks of a longer sequence, back to back (only the
    last may be short: the ragged last block of the sequence), q_scale [B,Hq,len(q_blocks)] their scales.  The causal mask and
    tile skipping use the absolute rows, so every row gets the bits of the same row of a full run.
    Rows are independent, so the loop runs over key tiles with all participating rows at once.
    Returns (o [B,Hq,Sq,D] fp32-valued rounded to out_dtype, lse [B,Hq,Sq] fp32 or None).
    """
    B, Hq, Sq, D = q_i8.shape
    _, Hkv, Sk, _ = k_i8.shape
    g = Hq // Hkv
    rows = _rows_of_blocks(q_blocks, Sq, BLOCK_M)  # absolute row indices
    if causal:
        assert (Sq == Sk) if q_blocks is None else (rows[-1] < Sk), "qo_len and kv_len must be equal for causal attention"  # causal :389
    n_kt = (Sk + BLOCK_N - 1) // BLOCK_N
    o = np.zeros((B, Hq, Sq, D), np.float32)
    lse = np.zeros((B, Hq, Sq), np.float32) if return_lse else None
    row_blk = np.arange(Sq) // BLOCK_M  # index into the given scales
    for b in range(B):
        for h in range(Hq):
            hk = h // g
            qf = q_i8[b, h].astype(np.float32)  # int8 products/sums < 2^24: exact in fp32
            kf = k_i8[b, hk].astype(np.float32)
            vf = v16[b, hk].astype(np.float16)
            qs = q_scale[b, h][row_blk].astype(np.float32)  # per-row copy of the per-block scale
            m_i = np.full(Sq, -np.inf, np.float32)
            l_i = np.ones(Sq, np.float32)  # :137  (erased by alpha=0 on the first tile)
            acc = np.zeros((Sq, D), np.float32)
            for j in range(n_kt):
                n0 = j * BLOCK_N
                n1 = min(n0 + BLOCK_N, Sk)
                if causal:
                    # q-tiles m with m*128 <= n0 take part: the given rows from the first one at or past that row on
                    r0 = int(np.searchsorted(rows, (n0 // BLOCK_M) * BLOCK_M))
                    if r0 >= Sq:
                        break
                else:
                    r0 = 0
                kt = kf[n0:n1]
                if n1 - n0 < BLOCK_N:  # masked load -> zeros
                    kt = np.concatenate([kt, np.zeros((BLOCK_N - (n1 - n0), D), np.float32)], 0)
                qk = (qf[r0:] @ kt.T).astype(np.float32)
                qk = qk * qs[r0:, None] * k_scale[b, hk, j]
                if n1 - n0 < BLOCK_N and tail == "neg_inf":
                    qk[:, n1 - n0:] = -np.inf
                if causal:
                    # rows of the diagonal q-tile (the given rows of block n0 // BLOCK_M) are masked
                    d1 = int(np.searchsorted(rows, (n0 // BLOCK_M + 1) * BLOCK_M))
                    rr = rows[r0:d1, None]
                    cc = (n0 + np.arange(BLOCK_N))[None, :]
                    if causal_mask == "neg_inf":
                        qk[: d1 - r0] = np.where(rr >= cc, qk[: d1 - r0], np.float32(-np.inf))
                    else:
                        qk[: d1 - r0] = qk[: d1 - r0] + np.where(rr >= cc, np.float32(0), np.float32(-1000000.0))
                m_ij = np.maximum(m_i[r0:], qk.max(axis=1))
                p = np.exp2(qk - m_ij[:, None]).astype(np.float32)
                l_ij = p.sum(axis=1, dtype=np.float32)
                alpha = np.exp2(m_i[r0:] - m_ij).astype(np.float32)
                l_i[r0:] = l_i[r0:] * alpha + l_ij
                acc[r0:] *= alpha[:, None]
                vt = vf[n0:n1]
                if n1 - n0 < BLOCK_N:
                    vt = np.concatenate([vt, np.zeros((BLOCK_N - (n1 - n0), D), np.float16)], 0)
                pv = p.astype(np.float16).astype(np.float32) @ vt.astype(np.float32)
                if pv_tile_fp16:
                    pv = pv.astype(np.float16).astype(np.float32)
                acc[r0:] += pv
                m_i[r0:] = m_ij
            o[b, h] = acc * (np.float32(1.0) / l_i)[:, None]
            if return_lse:
                lse[b, h] = np.log2(l_i) + m_i
    return to_storage(o, out_dtype), lse


# --------------------------------------------------------------------------------------
# fp8-PV variant (specification: csrc/qattn/qk_int_sv_f8_cuda.cu + csrc/fused/fused.cu) -- parity unpinned
# --------------------------------------------------------------------------------------
def per_channel_fp8(v: np.ndarray):
    """`per_channel_fp8` (src/quant.py:210-291) -> `MeanScaleKernel` (csrc/fused/fused.cu:317-428):
    per (b, h, d) channel: amax over tokens; scale = amax/448; v_fp8 = e4m3(v * 448/amax)
    (fused.cu:391-394,400,419-424).  v canonical [B,H,S,D] fp32-valued.
    Returns (v_fp8 values as fp32 [B,H,S,D], v_scale fp32 [B,H,D]).  The reference also
    transposes/pads/permutes V for its mma fragment (TransposePadPermuteKernel, fused.cu:263-314);
    that is a device layout choice, not arithmetic, and is not restated here.
    """
    amax = np.max(np.abs(v.astype(np.float32)), axis=2)  # [B,H,D]
    amax = np.maximum(amax, np.float32(1e-7))
    scale = (amax / np.float32(FP8_E4M3_MAX)).astype(np.float32)
    inv = (np.float32(FP8_E4M3_MAX) / amax).astype(np.float32)
    v8 = e4m3fn_round(v.astype(np.float32) * inv[:, :, None, :])
    return v8, scale


def attn_fwd_int8_fp8(q_i8, k_i8, v8, q_scale, k_scale, v_scale, *, causal: bool, out_dtype: str = "fp16",
                      return_lse: bool = False, BLOCK_M: int = 128, BLOCK_N: int = 64, return_slack: bool = False,
                      key_tiles_reversed=False, q_blocks=None):
    """`qk_int_sv_f8_attn_kernel` semantics (csrc/qattn/qk_int_sv_f8_cuda.cu:46-692) on per-block
    scales: p = exp2(s - m + 8.807) so that p_max = 448 (csrc/qattn/attn_utils.cuh:30,424-445);
    l += sum(p) in fp32 before the fp8 rounding (:314-317); p -> e4m3 satfinite RN
    (attn_utils.cuh:470-485); PV e4m3 x e4m3 -> fp32 accumulate; O = (acc/l) * v_scale (:554-579);
    lse = log2(l) + m - 8.807 (:689).  Out-of-range keys are masked with -inf (attn_utils.cuh:327-353)
    and the causal mask is exact (-inf above the diagonal).
    `return_slack`: also return `fp8_flip_slack(...)` (shaped like o, fp32, before the storage rounding); o and lse are
    computed by the same code either way.
    `key_tiles_reversed` (non-causal only): walk the 64-key tiles from the last to the first, as the HIP kernel does for every
    other round of 64 Q blocks (L2 reuse).  P is rounded to e4m3 against the RUNNING row maximum, so the order changes which
    references the codes are rounded against - by more than a rounding-boundary flip.  One bool for the call, or one per given
    Q block (the kernel's direction is a property of the block: `(qt // 64) & 1`).
    `q_blocks`: the given rows are these Q blocks of a longer sequence, as in `attn_fwd_int8_fp16`.
    """
    B, Hq, Sq, D = q_i8.shape
    split = _split_by_direction(q_blocks, q_scale.shape[2], key_tiles_reversed)
    if split is not None:
        kw = dict(k_i8=k_i8, v8=v8, k_scale=k_scale, v_scale=v_scale, causal=causal, out_dtype=out_dtype, return_lse=return_lse,
                  BLOCK_M=BLOCK_M, BLOCK_N=BLOCK_N, return_slack=return_slack)
        res = _by_direction(attn_fwd_int8_fp8, split, q_blocks, Sq, BLOCK_M, dict(q_i8=q_i8), dict(q_scale=q_scale), kw,
                            3 if return_slack else 2)
        return res
    key_tiles_reversed = bool(np.all(key_tiles_reversed))
    assert not (causal and key_tiles_reversed)
    _, Hkv, Sk, _ = k_i8.shape
    g = Hq // Hkv
    rows = _rows_of_blocks(q_blocks, Sq, BLOCK_M)  # absolute row indices
    if causal:
        assert (Sq == Sk) if q_blocks is None else (rows[-1] < Sk)
    n_kt = (Sk + BLOCK_N - 1) // BLOCK_N
    o = np.zeros((B, Hq, Sq, D), np.float32)
    lse = np.zeros((B, Hq, Sq), np.float32) if return_lse else None
    row_blk = np.arange(Sq) // BLOCK_M  # index into the given scales
    off = np.float32(FP8_P_OFFSET)
    for b in range(B):
        for h in range(Hq):
            hk = h // g
            qf = q_i8[b, h].astype(np.float32)
            kf = k_i8[b, hk].astype(np.float32)
            vf = v8[b, hk].astype(np.float32)
            qs = q_scale[b, h][row_blk].astype(np.float32)
            m_i = np.full(Sq, -np.inf, np.float32)
            l_i = np.zeros(Sq, np.float32)
            acc = np.zeros((Sq, D), np.float32)
            for j in (range(n_kt - 1, -1, -1) if key_tiles_reversed else range(n_kt)):
                n0 = j * BLOCK_N
                n1 = min(n0 + BLOCK_N, Sk)
                r0 = int(np.searchsorted(rows, (n0 // BLOCK_M) * BLOCK_M)) if causal else 0
                if r0 >= Sq:
                    break
                qk = (qf[r0:] @ kf[n0:n1].T).astype(np.float32)
                qk = qk * qs[r0:, None] * k_scale[b, hk, j]
                if causal:
                    cc = (n0 + np.arange(n1 - n0))[None, :]
                    qk = np.where(rows[r0:, None] >= cc, qk, -np.inf)
                m_ij = np.maximum(m_i[r0:], qk.max(axis=1))
                p = np.exp2(qk - m_ij[:, None] + off).astype(np.float32)
                alpha = np.exp2(m_i[r0:] - m_ij).astype(np.float32)
                l_i[r0:] = l_i[r0:] * alpha + p.sum(axis=1, dtype=np.float32)
                acc[r0:] *= alpha[:, None]
                acc[r0:] += e4m3fn_round(p) @ vf[n0:n1]
                m_i[r0:] = m_ij
            o[b, h] = acc / l_i[:, None] * v_scale[b, hk][None, :]
            if return_lse:
                lse[b, h] = np.log2(l_i) + m_i - off
    if return_slack:
        slack = fp8_flip_slack(q_i8, k_i8, v8, q_scale, k_scale, v_scale, o, causal=causal, BLOCK_M=BLOCK_M, BLOCK_N=BLOCK_N,
                               key_tiles_reversed=key_tiles_reversed, q_blocks=q_blocks)
        return to_storage(o, out_dtype), lse, slack
    return to_storage(o, out_dtype), lse


KMAGIC = 12582912.0  # 1.5 * 2^23: the bias a kernel may fold into its int32 scores (float(kMagic + s) == kMagic + s, |s| < 2^22)
GRID_WIDE_LOG2G = -6  # a kernel that folds the bias keeps its per-tile scale on a grid of G / 2^22 only while log2(G) < -6


def fp8_p_delta(S, M, A, sig, sig_m, same_tile, grid_g=None, s_int=None, t_int=None):
    """Largest difference (binades) between the exponent argument of a CORRECT fp8-PV kernel and the exact one,
    A = s sigma_j - t sigma_m + 8.807 (s, t integer scores, sigma = q_scale * k_scale as a real product; t, sigma_m those of the
    running row maximum M = t sigma_m; S = s sigma_j).  Every term is a rounding of an fp32 operand the kernel has to form:

      2^-22                       v_exp_f32: <= 1 ulp of P (2^-23 relative = 1.44 * 2^-23 binades)
      2^-22 (|A| + 8.807)         the fma that forms the argument and the add of 8.807 to its constant: two roundings of at most
                                  |A| + 8.807 each, 2^-24 per rounding, with a factor 2 so that +-2 ulps of the argument fit
      2^-23 (|M| [|M| < 2^16] + sigma_j)
                                  the row maximum rounded to fp32 (m_run) and the constant -m_run rounded again: 2 x 2^-24 |M|.
                                  Beyond 2^16 binades a kernel must keep the reference as an exact product (m_run + m_lo, the
                                  remainder form) - a reference rounded there moves P by percents - so the term drops out;
                                  what is left is the rounding of r sigma - m_run (r the integer nearest to m / sigma: <= sigma).
                                  (A reference taken while |M| < 2^16 and kept is covered by the first case.)
      2^-24 |S - M|   (same tile) the dequantisation scale q_scale * k_scale rounded to fp32 once: when the score and the row
      2^-24 (|S|+|M|) (otherwise) maximum come from the same key tile the SAME rounded scale multiplies both (the argument is
                                  (s - t) * sc), otherwise each product carries its own rounding
      grid (only while log2 G < -6, G = 2^(e + 1 - 21), 2^e <= 1.25 kMagic sigma_max < 2^(e+1), g = G 2^-22):
        (|s| e_g(sigma_j) + |t| e_g(sigma_m))   a kernel that folds kMagic into its scores keeps the scale on multiples of g:
                                  e_g(sigma) = g/2, or g - sigma where the grid rounds a tiny scale up to g
        2^-23 kMagic (sigma_j + g)  its constant c1 = -kMagic sc - m + 8.807 is rounded twice at the size of kMagic * sc: two
                                  half-ulps of that operand (one unit of the integer score times sigma, 1.5 sigma)

    The grid terms are the only ones that do not scale with 2^-24 of |A|, |S| or |M|: at N(0,1) inputs they dominate
    (sigma ~ 2^-12), and they are still a few ulps of the operand the kernel actually rounds, kMagic * sc.
    """
    S, M, A = np.abs(S), np.abs(M), np.abs(A)
    d = 2.0 ** -22 + 2.0 ** -22 * (A + FP8_P_OFFSET) + 2.0 ** -23 * (np.where(M < 2.0 ** 16, M, 0.0) + sig)
    d = d + 2.0 ** -24 * np.where(same_tile, np.abs(S - M), S + M)
    if grid_g is not None:
        g = grid_g

        def e_g(sg):
            return np.where(sg >= g / 2, g / 2, g - sg) + 2.0 ** -24 * sg
        d = d + np.abs(s_int) * e_g(sig) + np.abs(t_int) * e_g(sig_m) + 2.0 ** -23 * KMAGIC * (sig + g)
    return d


def _grid_step(sc_max32: np.float32):
    """g of a bias-folding kernel for the largest dequantisation scale of a (batch, kv-head, Q block), or None when the
    kernel dequantises un-rounded from the start (log2 G >= -6)."""
    x = np.float32(np.float32(1.25) * np.float32(np.float32(KMAGIC) * np.float32(sc_max32)))
    e = int(np.frexp(np.float64(x))[1]) - 1  # 2^e <= x < 2^(e+1)
    gexp = e + 1 - 21
    if gexp >= GRID_WIDE_LOG2G:
        return None
    return 2.0 ** (gexp - 22)


def fp8_flip_slack(q_i8, k_i8, v8, q_scale, k_scale, v_scale, o, *, causal: bool, BLOCK_M: int = 128, BLOCK_N: int = 64,
                   key_tiles_reversed=False, q_blocks=None):
    """Per-element bound on |O_kernel - O_oracle| that comes from the e4m3 rounding of P (`attn_fwd_int8_fp8`, fp8-PV).

    P = e4m3(exp2(A)) has 3 mantissa bits: an argument that differs by a few fp32 ulps moves P across a rounding boundary
    of e4m3 and flips its code by one step (1/16 .. 1/8 of P).  The oracle's fp32 argument A32 and a correct kernel's
    argument both lie near the EXACT argument A64 = s * (q_scale * k_scale) - M64 + 8.807, formed here in float64 from the
    integer score and the exact running row maximum; the kernel within delta = fp8_p_delta(...) of it (derivation there).
    So, per P:
      * flip   = max(code(A+), code(A32)) - min(code(A-), code(A32)),  A+- = max/min(A64, A32) +- delta
                 (every code the kernel may produce, and the oracle's code, lie in that range);
      * rowsum = P64 (2^delta - 1) + |P64 - P32|: how far the fp32 row sum l (summed BEFORE the e4m3 rounding) may move.
    Both are accumulated through the online-softmax rescales as acc and l are, and every rescale adds the error of its own
    factor alpha (kernel: 2^-22 + the reference errors before and after; oracle: its exact deviation) times what had been
    accumulated so far.  The result, in units of O:
        slack = (flip_acc / l) * v_scale + |o| * rowsum_acc / l
    i.e. the code flips moving the numerator, and a common factor 2^+-delta on P moving the row sum (this is what matters in
    one-hot rows, where the largest P saturates at 448 while l keeps the exact sum).  Everything else - fp32 accumulation
    order, one output ulp - is left to the checker's rtol / atol.  `key_tiles_reversed` and `q_blocks` as in
    `attn_fwd_int8_fp8`.  Returns fp32 [B, Hq, Sq, D].
    """
    B, Hq, Sq, D = q_i8.shape
    split = _split_by_direction(q_blocks, q_scale.shape[2], key_tiles_reversed)
    if split is not None:
        kw = dict(k_i8=k_i8, v8=v8, k_scale=k_scale, v_scale=v_scale, causal=causal, BLOCK_M=BLOCK_M, BLOCK_N=BLOCK_N)
        return _by_direction(fp8_flip_slack, split, q_blocks, Sq, BLOCK_M, dict(q_i8=q_i8, o=o), dict(q_scale=q_scale), kw, 1)[0]
    key_tiles_reversed = bool(np.all(key_tiles_reversed))
    _, Hkv, Sk, _ = k_i8.shape
    g = Hq // Hkv
    n_kt = (Sk + BLOCK_N - 1) // BLOCK_N
    slack = np.zeros((B, Hq, Sq, D), np.float32)
    rows = _rows_of_blocks(q_blocks, Sq, BLOCK_M)  # absolute row indices
    row_blk = np.arange(Sq) // BLOCK_M  # index into the given scales
    off = np.float32(FP8_P_OFFSET)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            for h in range(Hq):
                hk = h // g
                qf = q_i8[b, h].astype(np.float32)
                kf = k_i8[b, hk].astype(np.float32)
                va = np.abs(v8[b, hk].astype(np.float64))
                qs32 = q_scale[b, h][row_blk].astype(np.float32)
                ks32 = k_scale[b, hk].astype(np.float32)
                ks_max = np.float32(max(float(ks32.max()), 1e-30))
                grid = np.array([_grid_step(np.float32(x * ks_max)) or 0.0 for x in q_scale[b, h].astype(np.float32)])[row_blk]
                m32 = np.full(Sq, -np.inf, np.float32)          # the oracle's running max (fp32), as attn_fwd_int8_fp8
                m64 = np.full(Sq, -np.inf)                      # exact running max
                t_m = np.zeros(Sq)                              # its integer score, tile and scale
                j_m = np.full(Sq, -1)
                sig_m = np.zeros(Sq)
                l32 = np.zeros(Sq, np.float32)
                l64 = np.zeros(Sq)
                fl_acc = np.zeros((Sq, D))                      # sum |code_hi - code_lo| |v8|
                abs_acc = np.zeros((Sq, D))                     # sum code |v8|
                rs = np.zeros(Sq)                               # row-sum slack
                for j in (range(n_kt - 1, -1, -1) if key_tiles_reversed else range(n_kt)):
                    n0 = j * BLOCK_N
                    n1 = min(n0 + BLOCK_N, Sk)
                    r0 = int(np.searchsorted(rows, (n0 // BLOCK_M) * BLOCK_M)) if causal else 0
                    if r0 >= Sq:
                        break
                    R = slice(r0, Sq)
                    s_int = (qf[R] @ kf[n0:n1].T).astype(np.float64)
                    sig = qs32[R].astype(np.float64) * float(ks32[j])
                    qk32 = (qf[R] @ kf[n0:n1].T).astype(np.float32) * qs32[R, None] * ks32[j]
                    S64 = s_int * sig[:, None]
                    if causal:
                        live = rows[R, None] >= (n0 + np.arange(n1 - n0))[None, :]
                        qk32 = np.where(live, qk32, -np.inf)
                        S64 = np.where(live, S64, -np.inf)
                    # running maxima: the oracle's fp32 one and the exact one (with its integer score, tile and scale)
                    mo32 = m32[R]
                    mn32 = np.maximum(mo32, qk32.max(axis=1))
                    arg = np.argmax(S64, axis=1)
                    tmax = S64[np.arange(S64.shape[0]), arg]
                    mo64 = m64[R]
                    up = tmax > mo64
                    mn64 = np.where(up, tmax, mo64)
                    t_new = np.where(up, s_int[np.arange(S64.shape[0]), arg], t_m[R])
                    sigm_new = np.where(up, sig, sig_m[R])
                    jm_new = np.where(up, j, j_m[R])
                    gr = grid[R]
                    use_grid = gr > 0
                    # rescale of what was accumulated: the oracle's alpha and a kernel's, against the exact factor
                    prev = np.isfinite(mo64)
                    a32 = np.where(prev, np.exp2(mo32 - mn32), 0.0).astype(np.float32)
                    a64 = np.where(prev, np.exp2(mo64 - mn64), 0.0)
                    # error of a rescale (only where the maximum moved): a kernel's factor carries the reference errors
                    # before and after plus its exp2; the oracle's factor its own deviation from the exact one
                    e_old = fp8_p_delta(mo64, mo64, 0.0, sig_m[R], sig_m[R], False, gr, t_m[R], t_m[R])
                    e_new = fp8_p_delta(mn64, mn64, 0.0, sigm_new, sigm_new, False, gr, t_new, t_new)
                    e_old = np.where(use_grid, e_old, fp8_p_delta(mo64, mo64, 0.0, sig_m[R], sig_m[R], False))
                    e_new = np.where(use_grid, e_new, fp8_p_delta(mn64, mn64, 0.0, sigm_new, sigm_new, False))
                    dev_o = np.abs(np.log2(np.where(a32 > 0, a32, 1.0)) - (mo64 - mn64))
                    da = np.where(prev & up, 2.0 ** -22 + e_old + e_new + np.where(a32 > 0, dev_o, 0.0), 0.0)
                    grow = np.exp2(np.minimum(da, 64.0)) - 1.0  # (capped: finite, and far beyond any P ratio that matters)
                    fl_acc[R] = fl_acc[R] * a64[:, None] + np.where(abs_acc[R] > 0, grow[:, None] * abs_acc[R] * a64[:, None], 0.0)
                    rs[R] = rs[R] * a64 + np.where(l64[R] > 0, grow * l64[R] * a64, 0.0)
                    abs_acc[R] *= a64[:, None]
                    l64[R] *= a64
                    # P: the oracle's argument, the exact one, the window a kernel may use
                    A32 = (qk32 - mn32[:, None] + off).astype(np.float32)
                    A64 = S64 - mn64[:, None] + FP8_P_OFFSET
                    same = (jm_new == j)[:, None]
                    dk = fp8_p_delta(S64, mn64[:, None], A64, sig[:, None], sigm_new[:, None], same)
                    dkg = fp8_p_delta(S64, mn64[:, None], A64, sig[:, None], sigm_new[:, None], same, gr[:, None],
                                      s_int, t_new[:, None])
                    dk = np.where(use_grid[:, None], dkg, dk)
                    dead = ~np.isfinite(A64)
                    lo = np.where(dead, -np.inf, np.minimum(A64, A32) - dk)
                    hi = np.where(dead, -np.inf, np.maximum(A64, A32) + dk)
                    c_o = np.where(dead, 0.0, e4m3fn_round(np.exp2(np.where(dead, -np.inf, A32)).astype(np.float32)))
                    c_lo = e4m3fn_round(np.exp2(lo).astype(np.float32)).astype(np.float64)
                    c_hi = e4m3fn_round(np.exp2(np.minimum(hi, 30.0)).astype(np.float32)).astype(np.float64)
                    flip = np.maximum(c_hi, c_o) - np.minimum(c_lo, c_o)
                    p64 = np.where(dead, 0.0, np.exp2(np.where(dead, -np.inf, A64)))
                    p32 = np.exp2(np.where(dead, -np.inf, A32)).astype(np.float64)
                    rsj = np.where(dead | (p64 + p32 == 0), 0.0, p64 * (np.exp2(np.minimum(dk, 64.0)) - 1.0) + np.abs(p64 - p32))
                    fl_acc[R] += flip @ va[n0:n1]
                    abs_acc[R] += np.maximum(c_hi, c_o) @ va[n0:n1]
                    rs[R] += rsj.sum(axis=1)
                    l64[R] += p64.sum(axis=1)
                    l32[R] = l32[R] * a32 + p32.astype(np.float32).sum(axis=1, dtype=np.float32)
                    m32[R], m64[R], t_m[R], j_m[R], sig_m[R] = mn32, mn64, t_new, jm_new, sigm_new
                vs = v_scale[b, hk].astype(np.float64)[None, :]
                l_lo = np.minimum(l64, l32.astype(np.float64))[:, None]
                slack[b, h] = (fl_acc * vs + np.abs(o[b, h]).astype(np.float64) * rs[:, None]) / l_lo
    return slack


# --------------------------------------------------------------------------------------
# L3: the public operator  (src/core.py)
# --------------------------------------------------------------------------------------
def _canon(x: np.ndarray, tensor_layout: str) -> np.ndarray:
    """NHD [B,S,H,D] -> canonical [B,H,S,D].  The reference never copies: it swaps strides
    (src/triton/quant_per_block.py:188-203, src/triton/attn_qk_int8_per_block.py:183-196)."""
    if tensor_layout == "HND":
        return x
    if tensor_layout == "NHD":
        return np.transpose(x, (0, 2, 1, 3))
    raise ValueError(f"Unknown tensor layout: {tensor_layout}")


def _pad_head_dim(x: np.ndarray) -> np.ndarray:
    """src/core.py:277-287: D<64 -> 64, 64<D<128 -> 128 (zero pad), D>128 -> ValueError."""
    d = x.shape[-1]
    if d < 64:
        tgt = 64
    elif 64 < d < 128:
        tgt = 128
    elif d > 128:
        raise ValueError(f"Unsupported head_dim: {d}")
    else:
        return x
    pad = [(0, 0)] * (x.ndim - 1) + [(0, tgt - d)]
    return np.pad(x, pad)


def lowbit_fa_forward(q, k, v, *, dtype: str = "fp16", tensor_layout: str = "HND", is_causal: bool = False,
                      sm_scale=None, smooth_k: bool = True, return_lse: bool = False,
                      q_qmax: float = 127.0, k_qmax: float = 127.0, pv: str = "fp16",
                      tail: str = "reference", amax_floor: float = 0.0, pv_tile_fp16: bool = True,
                      return_intermediates: bool = False, return_slack: bool = False, causal_mask: str = "reference",
                      fp8_key_tiles_reversed=False, q_blocks=None):
    """`sageattn_qk_int8_pv_fp16_triton` (src/core.py:194-352); with q_qmax/k_qmax = 7 the intended
    semantics of `sageattn_qk_int4_pv_fp16_triton` (:945-1036, body defective - SURVEY 2.4-2/3); with
    pv='fp8' `sageattn_qk_int8_pv_fp8_cuda` (:735-941) on per-block scales.

    q, k, v: fp32-valued numpy arrays already rounded to `dtype` ('fp16'|'bf16'), in `tensor_layout`.
    Steps: pad D (:277-287); km = mean_S(k) (:292-293); lse_correction = q.km (:294-304);
    bf16 -> v.half() (:307-308); sm_scale = D_og^-0.5 (:309-310); quant (:311-320); attention
    (:321-342); slice (:343); lse/1.44269504 + lse_correction*sm_scale (:344-350).
    `return_slack` (pv='fp8' only): the e4m3 flip slack of O (`fp8_flip_slack`), laid out like o, is returned right after o.
    `q_blocks` (ascending 128-row block indices): q holds only the rows of these Q blocks of a longer sequence, back to back
    (`block_rows` gives them); k and v are whole.  km, the K / V codes and scales come from all keys, each Q block is quantised
    on its own, the causal mask uses absolute rows: o, lse (and the slack) are the bits of the same rows of a full run.
    `fp8_key_tiles_reversed`: one bool, or one per Q block (per given block with `q_blocks`).
    """
    if return_slack and pv != "fp8":
        raise ValueError("return_slack needs pv='fp8'")
    head_dim_og = q.shape[-1]
    q, k, v = _pad_head_dim(q), _pad_head_dim(k), _pad_head_dim(v)
    qc, kc, vc = _canon(q, tensor_layout), _canon(k, tensor_layout), _canon(v, tensor_layout)
    km = None
    lse_corr = None
    if smooth_k:
        km = mean_seq(kc, dtype)
        if return_lse:
            # matmul in the storage dtype, result rounded to it, then .to(float32) (:294-304)
            g = qc.shape[1] // kc.shape[1]
            kmq = np.repeat(km, g, axis=1) if g > 1 else km
            lse_corr = to_storage(np.einsum("bhsd,bhtd->bhs", qc.astype(np.float32), kmq.astype(np.float32)), dtype)
    v16 = vc.astype(np.float16).astype(np.float32)  # no-op for fp16 inputs (:307-308)
    if sm_scale is None:
        sm_scale = 1.0 / head_dim_og ** 0.5
    q_i8, q_scale, k_i8, k_scale = per_block_int8(qc, kc, km, sm_scale, dtype, q_qmax=q_qmax, k_qmax=k_qmax,
                                                  amax_floor=amax_floor)
    if pv == "fp16":
        o, lse = attn_fwd_int8_fp16(q_i8, k_i8, v16, q_scale, k_scale, causal=is_causal, out_dtype=dtype,
                                    return_lse=return_lse, tail=tail, pv_tile_fp16=pv_tile_fp16, causal_mask=causal_mask,
                                    q_blocks=q_blocks)
        v_scale = None
    elif pv == "fp8":
        v8, v_scale = per_channel_fp8(vc)
        res = attn_fwd_int8_fp8(q_i8, k_i8, v8, q_scale, k_scale, v_scale, causal=is_causal, out_dtype=dtype,
                                return_lse=return_lse, return_slack=return_slack, key_tiles_reversed=fp8_key_tiles_reversed,
                                q_blocks=q_blocks)
        o, lse = res[0], res[1]
        slack = res[2] if return_slack else None
    else:
        raise ValueError(pv)
    o = o[..., :head_dim_og]
    if tensor_layout == "NHD":
        o = np.ascontiguousarray(np.transpose(o, (0, 2, 1, 3)))
    if return_slack:
        slack = slack[..., :head_dim_og]
        if tensor_layout == "NHD":
            slack = np.ascontiguousarray(np.transpose(slack, (0, 2, 1, 3)))
    if return_lse:
        lse = lse / np.float32(LOG2E)
        if smooth_k:
            lse = lse + lse_corr * np.float32(sm_scale)
    head = (o, slack) if return_slack else (o,)
    if return_intermediates:
        return (*head, lse, dict(q_i8=q_i8, q_scale=q_scale, k_i8=k_i8, k_scale=k_scale, km=km, v_scale=v_scale))
    return (*head, lse) if return_lse else (head if return_slack else o)


# --------------------------------------------------------------------------------------
# Packed variable-length batches  (src/core.py:356-491)
# --------------------------------------------------------------------------------------
def lowbit_fa_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, *, dtype: str = "fp16", is_causal: bool = False,
                     sm_scale=None, smooth_k: bool = True, q_qmax: float = 127.0, k_qmax: float = 127.0,
                     tail: str = "reference", amax_floor: float = 0.0, return_intermediates: bool = False):
    """`sageattn_varlen` (src/core.py:356-491).  q [total_q, Hq, D], k / v [total_k, Hkv, D] fp32-valued arrays
    already rounded to `dtype`; cu_seqlens_* integer sequences of B + 1 entries.

    Steps: pad D (:431-440); bf16 -> v.half() (:449-450); km = k.mean(dim=0) over ALL packed tokens, k - km in
    the storage dtype (:451-454); sm_scale = D_og^-0.5 (:455-456); per sequence, with blocks restarting at the
    sequence start (src/triton/quant_per_block_varlen.py:41-72): Q * sm_scale*1.44269504 -> int8 per 128 rows,
    K -> int8 per 64 rows; per sequence the same tile loop as the dense kernel
    (src/triton/attn_qk_int8_block_varlen.py:24-92, causal: attn_qk_int8_per_block_causal_varlen.py:24-84);
    slice (:490).  Returns o [total_q, Hq, D_og] (and, on request, the packed codes and the scales in the
    reference layout [sum_blocks, H])."""
    head_dim_og = q.shape[-1]
    q, k, v = _pad_head_dim(q), _pad_head_dim(k), _pad_head_dim(v)
    cq = [int(x) for x in cu_seqlens_q]
    ck = [int(x) for x in cu_seqlens_k]
    assert len(cq) == len(ck)
    v16 = v.astype(np.float16).astype(np.float32)
    km = None
    if smooth_k:
        km = to_storage(np.mean(k.astype(np.float64), axis=0, keepdims=True).astype(np.float32), dtype)  # [1,Hkv,D]
        k = to_storage(k.astype(np.float32) - km.astype(np.float32), dtype)
    if sm_scale is None:
        sm_scale = 1.0 / head_dim_og ** 0.5
    o = np.zeros(q.shape, np.float32)
    q_i8 = np.zeros(q.shape, np.int8)
    k_i8 = np.zeros(k.shape, np.int8)
    q_scales, k_scales = [], []
    for b in range(len(cq) - 1):
        qb = np.transpose(q[cq[b]:cq[b + 1]], (1, 0, 2))[None]   # [1,Hq,len,D]
        kb = np.transpose(k[ck[b]:ck[b + 1]], (1, 0, 2))[None]
        vb = np.transpose(v16[ck[b]:ck[b + 1]], (1, 0, 2))[None]
        if qb.shape[2] == 0:
            continue
        qi, qs = quant_per_block(qb, np.float32(float(sm_scale) * LOG2E), q_qmax, 128, amax_floor)
        q_i8[cq[b]:cq[b + 1]] = np.transpose(qi[0], (1, 0, 2))
        q_scales.append(np.transpose(qs[0], (1, 0)))             # [blocks, Hq]
        if kb.shape[2] == 0:
            continue  # l = 1, acc = 0 -> zeros (attn_qk_int8_block_varlen.py:171-173)
        ki, ks = quant_per_block(kb, 1.0, k_qmax, 64, amax_floor)
        k_i8[ck[b]:ck[b + 1]] = np.transpose(ki[0], (1, 0, 2))
        k_scales.append(np.transpose(ks[0], (1, 0)))
        ob, _ = attn_fwd_int8_fp16(qi, ki, vb, qs, ks, causal=is_causal, out_dtype=dtype, return_lse=False, tail=tail)
        o[cq[b]:cq[b + 1]] = np.transpose(ob[0], (1, 0, 2))
    o = o[..., :head_dim_og]
    if return_intermediates:
        return o, dict(q_i8=q_i8, k_i8=k_i8, km=km,
                       q_scale=np.concatenate(q_scales, axis=0) if q_scales else np.zeros((0, q.shape[1]), np.float32),
                       k_scale=np.concatenate(k_scales, axis=0) if k_scales else np.zeros((0, k.shape[1]), np.float32))
    return o


def make_varlen_inputs(lens_q, lens_k, Hq, Hkv, D, *, seed=0, dtype="fp16", k_bias=0.0):
    """Seeded packed inputs: q [sum(lens_q), Hq, D], k / v [sum(lens_k), Hkv, D] ~ N(0,1) rounded to `dtype`."""
    rng = np.random.default_rng(seed)
    tq, tk = int(sum(lens_q)), int(sum(lens_k))
    q = to_storage(rng.standard_normal((tq, Hq, D), dtype=np.float32), dtype)
    k = to_storage(rng.standard_normal((tk, Hkv, D), dtype=np.float32) + np.float32(k_bias), dtype)
    v = to_storage(rng.standard_normal((tk, Hkv, D), dtype=np.float32), dtype)
    cu_q = np.concatenate([[0], np.cumsum(lens_q)]).astype(np.int32)
    cu_k = np.concatenate([[0], np.cumsum(lens_k)]).astype(np.int32)
    return q, k, v, cu_q, cu_k


# --------------------------------------------------------------------------------------
# CPU baseline: the repo's naive SDPA  (src/core.py:46-69)
# --------------------------------------------------------------------------------------
def sdpa_naive(q, k, v, is_causal: bool = False, sm_scale=None, return_lse: bool = False, q_blocks=None):
    """`manual_scaled_dot_product_attention` (src/core.py:46-69) with the intended K^T
    (`transpose([0,1,3,2])`; the reference's `[0,2,3,1]` at :55 is a bug):
    scores = q.k^T * D^-0.5 (:55); causal: scores += (1 - tril) * -1e9 (:58-61); softmax (:64); @ v (:67).
    Canonical [B,H,S,D]; GQA handled by repeating kv heads.  fp32 math (float64 when inputs are).
    `q_blocks`: q holds only the rows of these 128-row Q blocks of a longer sequence (as in `lowbit_fa_forward`); the causal
    mask uses their absolute rows."""
    B, Hq, Sq, D = q.shape
    Hkv = k.shape[1]
    if Hkv != Hq:
        k = np.repeat(k, Hq // Hkv, axis=1)
        v = np.repeat(v, Hq // Hkv, axis=1)
    scale = D ** -0.5 if sm_scale is None else sm_scale
    scores = np.matmul(q, np.swapaxes(k, -1, -2)) * q.dtype.type(scale)
    if is_causal:
        Sk = scores.shape[-1]
        if q_blocks is None:
            mask = np.tril(np.ones((Sq, Sk), dtype=scores.dtype))
        else:
            mask = (_rows_of_blocks(q_blocks, Sq)[:, None] >= np.arange(Sk)[None, :]).astype(scores.dtype)
        scores = scores + (1 - mask) * q.dtype.type(-1e9)
    mx = scores.max(axis=-1, keepdims=True)
    e = np.exp(scores - mx)
    s = e.sum(axis=-1, keepdims=True)
    out = np.matmul(e / s, v)
    if return_lse:
        return out, (np.log(s) + mx)[..., 0]
    return out


def sdpa_naive_torch(q, k, v, is_causal: bool = False, sm_scale=None):
    """The same `manual_scaled_dot_product_attention` (src/core.py:46-69) written with torch CPU tensor ops - the closest
    stand-in for the reference's Paddle-CPU path when Paddle is not installed (Paddle-CPU, else
    torch-CPU, else numpy).  q, k, v: torch CPU tensors [B,H,S,D].  Used for the CPU baseline timing only."""
    import torch
    D = q.shape[-1]
    scale = D ** -0.5 if sm_scale is None else sm_scale
    scores = torch.matmul(q, k.transpose(-1, -2)) * scale                      # :55 (intended K^T)
    if is_causal:
        Sq, Sk = scores.shape[-2], scores.shape[-1]
        mask = torch.tril(torch.ones((Sq, Sk), dtype=scores.dtype))            # :58-61
        scores = scores + (1 - mask) * -1e9
    return torch.matmul(torch.softmax(scores, dim=-1), v)                       # :64, :67


def attention_flops(B: int, H: int, Sq: int, Sk: int, D: int, causal: bool) -> float:
    """FLOP formula of the reference's bench harness: 4*B*H*D*S*S, halved for causal
    (utils/benchmark.py:212-214; example/test_sageattn_operator.py:96-98)."""
    f = 4.0 * B * H * D * Sq * Sk
    return f / 2 if causal else f


def make_inputs(B, H, S, D, *, seed=0, layout="HND", dtype="fp16", Hkv=None, Sk=None, k_bias=0.0, dist="normal"):
    """Seeded synthetic q,k,v: N(0,1) as example/test_sageattn_operator.py:43-52, or the bench
    distribution q,k = randint(-100,100), v ~ N(0,1) (utils/benchmark.py:215-230).  fp32-valued, rounded to dtype."""
    rng = np.random.default_rng(seed)
    Hkv = H if Hkv is None else Hkv
    Sk = S if Sk is None else Sk
    if dist == "normal":
        q = rng.standard_normal((B, H, S, D), dtype=np.float32)
        k = rng.standard_normal((B, Hkv, Sk, D), dtype=np.float32) + np.float32(k_bias)
    elif dist == "randint":
        q = rng.integers(-100, 100, (B, H, S, D)).astype(np.float32)
        k = rng.integers(-100, 100, (B, Hkv, Sk, D)).astype(np.float32) + np.float32(k_bias)
    else:
        raise ValueError(dist)
    v = rng.standard_normal((B, Hkv, Sk, D), dtype=np.float32)
    q, k, v = to_storage(q, dtype), to_storage(k, dtype), to_storage(v, dtype)
    if layout == "NHD":
        q, k, v = (np.ascontiguousarray(np.transpose(t, (0, 2, 1, 3))) for t in (q, k, v))
    return q, k, v
