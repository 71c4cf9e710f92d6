"""The refusals of the five decode entry points of csrc/decode.hip, called through _lib.lib() (CPU only: nothing is launched).
Every row of REFUSALS changes the valid call of its entry point in exactly one condition; the return code and the whole text of
mmgl_last_error() are literals recorded from the library before the entry points shared their checks, so the shared checks must
refuse every such call with the same code and the same words, the entry point's name included.
A pointer is None or an address that is never dereferenced (tests/test_decode_lora_cpu.py): every row fails before a launch.  With
a GPU visible the module skips -- there a check that went missing would turn its row into a launch on a made-up address."""
import pytest
import torch

P = 64        # a non-null, 16-byte aligned address that is never dereferenced
GEMM = dict(x=P, ldx=64, W=P, ldw=64, bias=None, residual=None, y=P, ldy=64, M=4, N=64, K=64, act=0, scale=1.0, dtype=1)
LORA = dict(GEMM, A=P, lda=64, B=P, ldb=8, r=8, lora_scale=2.0, ws=P)
ATTN = dict(q=P, ldq=64, k=P, v=P, ldkv=128, bs=1024, valid=P, ld_valid=8, out=P, B=2, H=4, S=8, D=16, dtype=1)
GQA = dict(ATTN, Hkv=2)
BEAM = dict(ATTN, kt=P, vt=P, ld_tail=128, rs_tail=512, src=P, ld_src=4, W=3, n_tail=2)

# entry point -> (its valid call, the order of its arguments; the stream, always null, comes last)
ENTRY = {
    "mmgl_gemm_skinny": (GEMM, "x ldx W ldw bias residual y ldy M N K act scale dtype"),
    "mmgl_gemm_skinny_lora": (LORA, "x ldx W ldw bias residual y ldy A lda B ldb r lora_scale ws M N K act scale dtype"),
    "mmgl_attn_decode_fwd": (ATTN, "q ldq k v ldkv bs valid ld_valid out B H S D dtype"),
    "mmgl_attn_decode_gqa_fwd": (GQA, "q ldq k v ldkv bs valid ld_valid out B H Hkv S D dtype"),
    "mmgl_attn_decode_beam_fwd": (BEAM, "q ldq k v ldkv bs valid ld_valid kt vt ld_tail rs_tail src ld_src out B W H S n_tail D dtype"),
}

# (entry point, the one condition violated, the arguments changed for it, return code, mmgl_last_error())
REFUSALS = [
    ('mmgl_gemm_skinny', 'sizes', dict(M=0), 1, 'mmgl_gemm_skinny: bad sizes M=0 N=64 K=64'),
    ('mmgl_gemm_skinny', 'M = 65', dict(M=65), 2, 'mmgl_gemm_skinny: M=65 > 64 rows (chunk the rows or use mmgl_gemm_nt)'),
    ('mmgl_gemm_skinny', 'dtype', dict(dtype=7), 1, 'mmgl_gemm_skinny: bad dtype 7'),
    ('mmgl_gemm_skinny', 'null x', dict(x=None), 1, 'mmgl_gemm_skinny: null pointer'),
    ('mmgl_gemm_skinny', 'null y', dict(y=None), 1, 'mmgl_gemm_skinny: null pointer'),
    ('mmgl_gemm_skinny', 'activation', dict(act=5), 1, 'mmgl_gemm_skinny: unknown activation 5'),
    ('mmgl_gemm_skinny', 'ldx', dict(ldx=63), 1, 'mmgl_gemm_skinny: leading dimensions (63, 64, 64) smaller than the rows (K=64, N=64)'),
    ('mmgl_gemm_skinny', 'ldy', dict(ldy=63), 1, 'mmgl_gemm_skinny: leading dimensions (64, 64, 63) smaller than the rows (K=64, N=64)'),
    ('mmgl_gemm_skinny_lora', 'sizes', dict(M=0), 1, 'mmgl_gemm_skinny_lora: bad sizes M=0 N=64 K=64 r=8'),
    ('mmgl_gemm_skinny_lora', 'M = 65', dict(M=65), 2, 'mmgl_gemm_skinny_lora: M=65 > 64 rows (chunk the rows)'),
    ('mmgl_gemm_skinny_lora', 'dtype', dict(dtype=7), 1, 'mmgl_gemm_skinny_lora: bad dtype 7'),
    ('mmgl_gemm_skinny_lora', 'null x', dict(x=None), 1, 'mmgl_gemm_skinny_lora: null pointer'),
    ('mmgl_gemm_skinny_lora', 'null lora_B', dict(B=None), 1, 'mmgl_gemm_skinny_lora: null pointer'),
    ('mmgl_gemm_skinny_lora', 'null workspace', dict(ws=None), 1, 'mmgl_gemm_skinny_lora: null pointer'),
    ('mmgl_gemm_skinny_lora', 'activation', dict(act=5), 1, 'mmgl_gemm_skinny_lora: unknown activation 5'),
    ('mmgl_gemm_skinny_lora', 'ldw', dict(ldw=63), 1, 'mmgl_gemm_skinny_lora: leading dimensions (64, 63, 64, 64, 8) smaller than the rows (K=64, N=64, r=8)'),
    ('mmgl_gemm_skinny_lora', 'ldb', dict(ldb=7), 1, 'mmgl_gemm_skinny_lora: leading dimensions (64, 64, 64, 64, 7) smaller than the rows (K=64, N=64, r=8)'),
    ('mmgl_gemm_skinny_lora', 'r = 0', dict(r=0), 1, 'mmgl_gemm_skinny_lora: bad sizes M=4 N=64 K=64 r=0'),
    ('mmgl_gemm_skinny_lora', 'r = 257', dict(r=257, ldb=264), 2, 'mmgl_gemm_skinny_lora: rank 257 > 256'),
    ('mmgl_gemm_skinny_lora', 'workspace alignment', dict(ws=66), 1, 'mmgl_gemm_skinny_lora: the fp32 workspace is not 4-byte aligned'),
    ('mmgl_attn_decode_fwd', 'sizes', dict(B=0), 1, 'mmgl_attn_decode_fwd: bad sizes B=0 H=4 S=8'),
    ('mmgl_attn_decode_fwd', 'sizes S', dict(S=0), 1, 'mmgl_attn_decode_fwd: bad sizes B=2 H=4 S=0'),
    ('mmgl_attn_decode_fwd', 'dtype', dict(dtype=7), 1, 'mmgl_attn_decode_fwd: bad dtype 7'),
    ('mmgl_attn_decode_fwd', 'head_dim 48', dict(D=48, ldq=192, ldkv=384, bs=3072), 2, 'mmgl_attn_decode_fwd: head_dim 48 (16, 32, 64, 128)'),
    ('mmgl_attn_decode_fwd', 'ldq no 16-byte multiple', dict(ldq=68), 2, 'mmgl_attn_decode_fwd: strides (68, 128, 1024) must be multiples of 16 bytes'),
    ('mmgl_attn_decode_fwd', 'batch stride no 16-byte multiple, fp32', dict(dtype=0, bs=1026), 2, 'mmgl_attn_decode_fwd: strides (64, 128, 1026) must be multiples of 16 bytes'),
    ('mmgl_attn_decode_fwd', 'null q', dict(q=None), 1, 'mmgl_attn_decode_fwd: null pointer'),
    ('mmgl_attn_decode_fwd', 'null mask', dict(valid=None), 1, 'mmgl_attn_decode_fwd: null pointer'),
    ('mmgl_attn_decode_fwd', 'ldq smaller than the row', dict(ldq=56), 1, 'mmgl_attn_decode_fwd: strides (56, 128, 8) smaller than the rows'),
    ('mmgl_attn_decode_fwd', 'mask stride smaller than the row', dict(ld_valid=7), 1, 'mmgl_attn_decode_fwd: strides (64, 128, 7) smaller than the rows'),
    ('mmgl_attn_decode_fwd', 'misaligned q', dict(q=72), 2, 'mmgl_attn_decode_fwd: q, k and v must be 16-byte aligned'),
    ('mmgl_attn_decode_fwd', 'misaligned k', dict(k=72), 2, 'mmgl_attn_decode_fwd: q, k and v must be 16-byte aligned'),
    ('mmgl_attn_decode_fwd', '2 GiB span', dict(S=8388609, ld_valid=8388609, bs=1073741952), 2, "mmgl_attn_decode_fwd: a sample's key rows span 2 GiB or more (S=8388609, ldkv=128)"),
    ('mmgl_attn_decode_fwd', '2 GiB span, fp32', dict(dtype=0, S=4194305, ld_valid=8388609, bs=1073741952), 2, "mmgl_attn_decode_fwd: a sample's key rows span 2 GiB or more (S=4194305, ldkv=128)"),
    ('mmgl_attn_decode_fwd', 'ldkv smaller than the row', dict(ldkv=56), 1, 'mmgl_attn_decode_fwd: strides (64, 56, 8) smaller than the rows'),
    ('mmgl_attn_decode_gqa_fwd', 'sizes', dict(B=0), 1, 'mmgl_attn_decode_gqa_fwd: bad sizes B=0 H=4 Hkv=2 S=8'),
    ('mmgl_attn_decode_gqa_fwd', 'sizes S', dict(S=0), 1, 'mmgl_attn_decode_gqa_fwd: bad sizes B=2 H=4 Hkv=2 S=0'),
    ('mmgl_attn_decode_gqa_fwd', 'dtype', dict(dtype=7), 1, 'mmgl_attn_decode_gqa_fwd: bad dtype 7'),
    ('mmgl_attn_decode_gqa_fwd', 'head_dim 48', dict(D=48, ldq=192, ldkv=384, bs=3072), 2, 'mmgl_attn_decode_gqa_fwd: head_dim 48 (16, 32, 64, 128)'),
    ('mmgl_attn_decode_gqa_fwd', 'ldq no 16-byte multiple', dict(ldq=68), 2, 'mmgl_attn_decode_gqa_fwd: strides (68, 128, 1024) must be multiples of 16 bytes'),
    ('mmgl_attn_decode_gqa_fwd', 'batch stride no 16-byte multiple, fp32', dict(dtype=0, bs=1026), 2, 'mmgl_attn_decode_gqa_fwd: strides (64, 128, 1026) must be multiples of 16 bytes'),
    ('mmgl_attn_decode_gqa_fwd', 'null q', dict(q=None), 1, 'mmgl_attn_decode_gqa_fwd: null pointer'),
    ('mmgl_attn_decode_gqa_fwd', 'null mask', dict(valid=None), 1, 'mmgl_attn_decode_gqa_fwd: null pointer'),
    ('mmgl_attn_decode_gqa_fwd', 'ldq smaller than the row', dict(ldq=56), 1, 'mmgl_attn_decode_gqa_fwd: strides (56, 128, 8) smaller than the rows'),
    ('mmgl_attn_decode_gqa_fwd', 'mask stride smaller than the row', dict(ld_valid=7), 1, 'mmgl_attn_decode_gqa_fwd: strides (64, 128, 7) smaller than the rows'),
    ('mmgl_attn_decode_gqa_fwd', 'misaligned q', dict(q=72), 2, 'mmgl_attn_decode_gqa_fwd: q, k and v must be 16-byte aligned'),
    ('mmgl_attn_decode_gqa_fwd', 'misaligned k', dict(k=72), 2, 'mmgl_attn_decode_gqa_fwd: q, k and v must be 16-byte aligned'),
    ('mmgl_attn_decode_gqa_fwd', '2 GiB span', dict(S=8388609, ld_valid=8388609, bs=1073741952), 2, "mmgl_attn_decode_gqa_fwd: a sample's key rows span 2 GiB or more (S=8388609, ldkv=128)"),
    ('mmgl_attn_decode_gqa_fwd', '2 GiB span, fp32', dict(dtype=0, S=4194305, ld_valid=8388609, bs=1073741952), 2, "mmgl_attn_decode_gqa_fwd: a sample's key rows span 2 GiB or more (S=4194305, ldkv=128)"),
    ('mmgl_attn_decode_gqa_fwd', 'sizes Hkv', dict(Hkv=0), 1, 'mmgl_attn_decode_gqa_fwd: bad sizes B=2 H=4 Hkv=0 S=8'),
    ('mmgl_attn_decode_gqa_fwd', 'H % Hkv', dict(Hkv=3), 1, 'mmgl_attn_decode_gqa_fwd: 4 query heads are no multiple of 3 key/value heads'),
    ('mmgl_attn_decode_gqa_fwd', 'ldkv smaller than the row', dict(ldkv=24), 1, 'mmgl_attn_decode_gqa_fwd: strides (64, 24, 8) smaller than the rows'),
    ('mmgl_attn_decode_beam_fwd', 'sizes', dict(B=0), 1, 'mmgl_attn_decode_beam_fwd: bad sizes B=0 W=3 H=4 S_pre=8 n_tail=2'),
    ('mmgl_attn_decode_beam_fwd', 'sizes S', dict(S=0), 1, 'mmgl_attn_decode_beam_fwd: bad sizes B=2 W=3 H=4 S_pre=0 n_tail=2'),
    ('mmgl_attn_decode_beam_fwd', 'dtype', dict(dtype=7), 1, 'mmgl_attn_decode_beam_fwd: bad dtype 7'),
    ('mmgl_attn_decode_beam_fwd', 'head_dim 48', dict(D=48, ldq=192, ldkv=384, bs=3072), 2, 'mmgl_attn_decode_beam_fwd: head_dim 48 (16, 32, 64, 128)'),
    ('mmgl_attn_decode_beam_fwd', 'ldq no 16-byte multiple', dict(ldq=68), 2, 'mmgl_attn_decode_beam_fwd: strides (68, 128, 1024) must be multiples of 16 bytes'),
    ('mmgl_attn_decode_beam_fwd', 'batch stride no 16-byte multiple, fp32', dict(dtype=0, bs=1026), 2, 'mmgl_attn_decode_beam_fwd: strides (64, 128, 1026) must be multiples of 16 bytes'),
    ('mmgl_attn_decode_beam_fwd', 'null q', dict(q=None), 1, 'mmgl_attn_decode_beam_fwd: null pointer'),
    ('mmgl_attn_decode_beam_fwd', 'null mask', dict(valid=None), 1, 'mmgl_attn_decode_beam_fwd: null pointer'),
    ('mmgl_attn_decode_beam_fwd', 'ldq smaller than the row', dict(ldq=56), 1, 'mmgl_attn_decode_beam_fwd: strides (56, 128, 8) smaller than the rows'),
    ('mmgl_attn_decode_beam_fwd', 'mask stride smaller than the row', dict(ld_valid=7), 1, 'mmgl_attn_decode_beam_fwd: strides (64, 128, 7) smaller than the rows'),
    ('mmgl_attn_decode_beam_fwd', 'misaligned q', dict(q=72), 2, 'mmgl_attn_decode_beam_fwd: q, k_pre and v_pre must be 16-byte aligned'),
    ('mmgl_attn_decode_beam_fwd', 'misaligned k', dict(k=72), 2, 'mmgl_attn_decode_beam_fwd: q, k_pre and v_pre must be 16-byte aligned'),
    ('mmgl_attn_decode_beam_fwd', '2 GiB span', dict(S=8388609, ld_valid=8388609, bs=1073741952), 2, "mmgl_attn_decode_beam_fwd: a sample's prefix rows span 2 GiB or more (S_pre=8388609, ld_pre=128)"),
    ('mmgl_attn_decode_beam_fwd', '2 GiB span, fp32', dict(dtype=0, S=4194305, ld_valid=8388609, bs=1073741952), 2, "mmgl_attn_decode_beam_fwd: a sample's prefix rows span 2 GiB or more (S_pre=4194305, ld_pre=128)"),
    ('mmgl_attn_decode_beam_fwd', 'ldkv smaller than the row', dict(ldkv=56), 1, 'mmgl_attn_decode_beam_fwd: strides (64, 56, 8) smaller than the rows'),
    ('mmgl_attn_decode_beam_fwd', 'sizes n_tail', dict(n_tail=-1), 1, 'mmgl_attn_decode_beam_fwd: bad sizes B=2 W=3 H=4 S_pre=8 n_tail=-1'),
    ('mmgl_attn_decode_beam_fwd', 'W = 9', dict(W=9), 2, 'mmgl_attn_decode_beam_fwd: 9 beams per sample (1..8)'),
    ('mmgl_attn_decode_beam_fwd', 'null tail', dict(kt=None), 1, 'mmgl_attn_decode_beam_fwd: null tail pointer with n_tail=2'),
    ('mmgl_attn_decode_beam_fwd', 'null src', dict(src=None), 1, 'mmgl_attn_decode_beam_fwd: null tail pointer with n_tail=2'),
    ('mmgl_attn_decode_beam_fwd', 'tail stride no 16-byte multiple', dict(ld_tail=132), 2, 'mmgl_attn_decode_beam_fwd: tail strides (132, 512) must be multiples of 16 bytes, k_tail and v_tail 16-byte aligned, src 4-byte'),
    ('mmgl_attn_decode_beam_fwd', 'misaligned v_tail', dict(vt=72), 2, 'mmgl_attn_decode_beam_fwd: tail strides (128, 512) must be multiples of 16 bytes, k_tail and v_tail 16-byte aligned, src 4-byte'),
    ('mmgl_attn_decode_beam_fwd', 'misaligned src', dict(src=66), 2, 'mmgl_attn_decode_beam_fwd: tail strides (128, 512) must be multiples of 16 bytes, k_tail and v_tail 16-byte aligned, src 4-byte'),
    ('mmgl_attn_decode_beam_fwd', 'ld_tail smaller than the row', dict(ld_tail=56), 1, 'mmgl_attn_decode_beam_fwd: tail strides (56, 512, 4) smaller than the rows'),
    ('mmgl_attn_decode_beam_fwd', 'ld_src smaller than the row', dict(ld_src=1), 1, 'mmgl_attn_decode_beam_fwd: tail strides (128, 512, 1) smaller than the rows'),
    ('mmgl_attn_decode_beam_fwd', 'tail row stride smaller than its rows', dict(rs_tail=128), 1, 'mmgl_attn_decode_beam_fwd: tail strides (128, 128, 4) smaller than the rows'),
    ('mmgl_attn_decode_beam_fwd', 'tail span', dict(rs_tail=1073741824), 2, "mmgl_attn_decode_beam_fwd: a sample's tail rows span 2 GiB or more (W=3, row stride 1073741824)"),
]


@pytest.mark.parametrize("fn,what,change,code,text", REFUSALS, ids=[f"{r[0]}-{r[1]}" for r in REFUSALS])
def test_decode_entry_point_refuses(fn, what, change, code, text):
    if torch.cuda.is_available():
        pytest.skip("runs where no GPU is visible: a missing check would launch on a made-up address")
    from mmgl_amd import _lib
    L = _lib.lib()
    valid, order = ENTRY[fn]
    assert set(change) <= set(valid)
    args = dict(valid, **change)
    assert getattr(L, fn)(*[args[name] for name in order.split()], None) == code
    assert L.mmgl_last_error().decode() == text
