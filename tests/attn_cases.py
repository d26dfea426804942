"""Hand-labelled routing cases of the attention kernels: which kernel
maeclip_attn_fwd / maeclip_attn_bwd run a call on (maeclip::AttnPath, the
number maeclip_attn_impl returns) or the message they reject it with. The
labels follow the documented rules (include/maeclip.h, DESIGN.md "Attention
routing") and the LDS footprints worked out by hand below, not a run of the
code. test_attention_route_cpu.py asks the library for every case without a
GPU; the GPU tests assert the path of a call before they compare its numbers.

LDS footprints (bytes; 160 KiB = 163840; image rows are 2 hd bytes in bf16 and
4 hd + 16 in fp32; npad rounds n up to 64 in the forward, to 32 in the backward):
  forward         2 npad row + 4 npad                      (+ a third image: fwd_qimg)
  backward, two   2 npad row + 8 npad + 12 hd nw           (fp32 always two)
  backward, four  4 npad row + 8 npad + 12 hd nw
  diagonal        2 npad row + 8 npad + 4 hd npad + 64 npad + hd npad + npad / 8
"""
import ctypes
from dataclasses import dataclass, field

FWD, FWD16, BWD_FOUR, BWD_TWO, BWD_TWO3, BWD_MASKED, BWD_DIAG, BWD_16, ROWS, STREAM, BWD_OCC = range(11)
NAMES = ("FWD", "FWD16", "BWD_FOUR", "BWD_TWO", "BWD_TWO3", "BWD_MASKED", "BWD_DIAG", "BWD_16", "ROWS", "STREAM",
         "BWD_OCC")
ATTN_OPTS = ("ATTN_TWO", "ATTN_ROWS", "ATTN_DIAG", "ATTN_BW16", "ATTN_FW16", "ATTN_STREAM")

_BUF = (ctypes.c_float * 64)()


def _ptr():
    p = ctypes.cast(_BUF, ctypes.c_void_p).value
    return (p + 15) & ~15   # the fp8-blocks copy wants 16-byte alignment; never dereferenced


def attn_args(dtype, n, H, hd, B=1, key_mask=False, dropout_p=0.0, q8=False, bwd=False, ld_qkv=None):
    """maeclip_attn_args of a dense call with dummy host pointers (the route never reads them)"""
    from mae_clip_amd import _lib as L
    p, D = _ptr(), H * hd
    return L.AttnArgs(qkv=p, o=p, lse=p, dout=p, dqkv=p, key_mask=p if key_mask else None, colsum_partial=None,
                      ld_qkv=ld_qkv or 3 * D, ld_o=D, ld_dqkv=3 * D, B=B, n=n, H=H, head_dim=hd,
                      dtype=L.BF16 if dtype == "bf16" else L.F32, scale=hd ** -0.5, dropout_p=dropout_p, seed=0,
                      step_ptr=None, q8=p if q8 else None, ldq8=(3 if bwd else 1) * D if q8 else 0,
                      q8_scale=p if q8 else None, q8_fmt=2 if q8 else 0)   # MAECLIP_FP8_E4M3


def impl(dtype, n, H, hd, bwd, **kw):
    """(path, message) the library gives under the options set now; dtype "bf16" / "f32" or a torch dtype"""
    from mae_clip_amd import _lib as L
    lib = L.load()
    name = dtype if isinstance(dtype, str) else ("bf16" if "bfloat16" in str(dtype) else "f32")
    a = attn_args(name, n, H, hd, bwd=bwd, **kw)
    rc = lib.maeclip_attn_impl(ctypes.byref(a), 1 if bwd else 0)
    return rc, (lib.maeclip_last_error() if rc < 0 else b"")


def path(dtype, n, H, hd, bwd, **kw):
    rc, msg = impl(dtype, n, H, hd, bwd, **kw)
    assert rc >= 0, msg
    return rc


@dataclass
class Case:
    id: str
    dtype: str            # "bf16" / "f32"
    hd: int
    n: int
    bwd: bool
    expect: object        # a path number, or the bytes a rejection's message holds
    H: int = 2
    kw: dict = field(default_factory=dict)     # key_mask, dropout_p, q8, ld_qkv
    opts: dict = field(default_factory=dict)   # ATTN_* options; the others unset


def cases():
    F, B_ = False, True
    c = []

    def add(id, dtype, hd, n, bwd, expect, opts=None, **kw):
        c.append(Case(id, dtype, hd, n, bwd, expect, H=kw.pop("H", 2), kw=kw, opts=opts or {}))

    # ---- streamed limit, no option set. hd 64: the forward's two images are 260 npad: 149760 at npad 576,
    # 166400 at 640; the backward's two at 8 waves 264 npad + 6144: 158208 at 576, 166656 at 608.
    # Below it: 36 tiles and one workgroup per CU -> the 16-wave forward; the backward by occupancy.
    add("stream_fwd64_576", "bf16", 64, 576, F, FWD16)
    add("stream_fwd64_577", "bf16", 64, 577, F, STREAM)
    add("stream_bwd64_576", "bf16", 64, 576, B_, BWD_OCC)
    add("stream_bwd64_577", "bf16", 64, 577, B_, STREAM)
    # hd 32 forward 132 npad: 160512 at 1216, 168960 at 1280; backward 136 npad + 3072: 159744 at 1152, 164096 at 1184
    add("stream_fwd32_1216", "bf16", 32, 1216, F, FWD16)
    add("stream_fwd32_1217", "bf16", 32, 1217, F, STREAM)
    add("stream_bwd32_1152", "bf16", 32, 1152, B_, BWD_16)   # 16 waves: 136 * 1152 + 6144 = 162816
    add("stream_bwd32_1153", "bf16", 32, 1153, B_, STREAM)
    add("stream_fwd32_1153", "bf16", 32, 1153, F, FWD16)     # forward and backward decide independently
    # ATTN_STREAM 1 / 0
    add("stream_on_fwd_25", "bf16", 64, 25, F, STREAM, {"ATTN_STREAM": 1})
    add("stream_on_bwd_25", "bf16", 64, 25, B_, STREAM, {"ATTN_STREAM": 1})
    add("stream_on_f32_ignored", "f32", 64, 25, F, FWD, {"ATTN_STREAM": 1})
    add("stream_off_fwd_700", "bf16", 64, 700, F, b"maeclip_attn: n=700 needs", {"ATTN_STREAM": 0})
    add("stream_off_bwd_700", "bf16", 64, 700, B_, b"of LDS (> 160 KiB)", {"ATTN_STREAM": 0})
    add("stream_off_fwd_577", "bf16", 64, 577, F, b"maeclip_attn: n=577 needs 166400 B", {"ATTN_STREAM": 0})
    # ATTN_TWO = 0 pins four images, 520 npad + 6144 at hd 64: 155904 at npad 288, 172544 at 320
    add("stream_two0_bwd64_288", "bf16", 64, 288, B_, BWD_FOUR, {"ATTN_TWO": 0})
    add("stream_two0_bwd64_289", "bf16", 64, 289, B_, STREAM, {"ATTN_TWO": 0})
    add("stream_unset_bwd64_289", "bf16", 64, 289, B_, BWD_OCC)
    # the streamed path's own rejections
    add("stream_mask_fwd", "bf16", 64, 700, F, b"streamed path", key_mask=True)
    add("stream_dropout_bwd", "bf16", 64, 700, B_, b"takes no key_mask and no dropout", dropout_p=0.1)
    add("stream_span", "bf16", 64, 700, F, b"must span less than 2 GiB", ld_qkv=1 << 21)

    # ---- diagonal backward. hd 32 (104 npad + npad / 8 ... 92192 at npad 256): on up to npad 256
    add("diag32_256", "bf16", 32, 256, B_, BWD_DIAG)
    add("diag32_257", "bf16", 32, 257, B_, BWD_16)           # 17 tiles: the 16-wave backward is hd 32's default
    add("diag32_off", "bf16", 32, 197, B_, BWD_16, {"ATTN_DIAG": 0})
    add("diag32_off_bw16_off", "bf16", 32, 197, B_, BWD_OCC, {"ATTN_DIAG": 0, "ATTN_BW16": 0})
    add("diag32_small", "bf16", 32, 5, B_, BWD_DIAG)
    # hd 64: default from npad 192 (n 161) to npad 224 (145180 B); npad 256 is 165920 B
    add("diag64_160", "bf16", 64, 160, B_, BWD_OCC)          # 10 tiles, but the 16-wave backward is off at hd 64
    add("diag64_161", "bf16", 64, 161, B_, BWD_DIAG)
    add("diag64_224", "bf16", 64, 224, B_, BWD_DIAG)
    add("diag64_225", "bf16", 64, 225, B_, BWD_OCC)
    add("diag64_on_50", "bf16", 64, 50, B_, BWD_DIAG, {"ATTN_DIAG": 1})
    add("diag64_on_225_lds", "bf16", 64, 225, B_, BWD_OCC, {"ATTN_DIAG": 1})
    add("diag64_off_197", "bf16", 64, 197, B_, BWD_OCC, {"ATTN_DIAG": 0})
    add("diag64_mask_197", "bf16", 64, 197, B_, BWD_MASKED, key_mask=True)
    add("diag64_on_mask_197", "bf16", 64, 197, B_, BWD_MASKED, {"ATTN_DIAG": 1}, key_mask=True)
    add("diag_f32_never", "f32", 32, 197, B_, BWD_FOUR, {"ATTN_DIAG": 1})

    # ---- 16-wave backward: more than 8 tiles; default at hd 32, hd 64 only when forced
    add("bw16_64_default_257", "bf16", 64, 257, B_, BWD_OCC)
    add("bw16_64_on_257", "bf16", 64, 257, B_, BWD_16, {"ATTN_BW16": 1})
    add("bw16_64_on_197", "bf16", 64, 197, B_, BWD_16, {"ATTN_BW16": 1, "ATTN_DIAG": 0})
    add("bw16_64_on_197_diag_first", "bf16", 64, 197, B_, BWD_DIAG, {"ATTN_BW16": 1})
    add("bw16_32_off_257", "bf16", 32, 257, B_, BWD_OCC, {"ATTN_BW16": 0})
    add("bw16_8_tiles", "bf16", 32, 128, B_, BWD_OCC, {"ATTN_BW16": 1, "ATTN_DIAG": 0})
    add("bw16_9_tiles", "bf16", 32, 129, B_, BWD_16, {"ATTN_BW16": 1, "ATTN_DIAG": 0})
    # its LDS at hd 64, 264 npad + 12288: 155904 at npad 544, 164352 at 576 -> the 8-wave kernels
    add("bw16_64_lds_544", "bf16", 64, 544, B_, BWD_16, {"ATTN_BW16": 1})
    add("bw16_64_lds_576", "bf16", 64, 576, B_, BWD_OCC, {"ATTN_BW16": 1})
    add("bw16_64_lds_576_two", "bf16", 64, 576, B_, BWD_TWO, {"ATTN_BW16": 1, "ATTN_TWO": 1})

    # ---- 16-wave forward: more than 8 tiles and 2 x LDS > 160 KiB
    add("fw16_32_576", "bf16", 32, 576, F, FWD)              # 76032 B
    add("fw16_32_577", "bf16", 32, 577, F, FWD16)            # 84480 B
    add("fw16_32_577_off", "bf16", 32, 577, F, FWD, {"ATTN_FW16": 0})
    add("fw16_64_256", "bf16", 64, 256, F, FWD)              # 66560 B
    add("fw16_64_257", "bf16", 64, 257, F, FWD16)            # 83200 B
    add("fw16_8_tiles", "bf16", 64, 128, F, FWD)
    add("fw16_f32_64_130", "f32", 64, 130, F, FWD16)         # 548 * 192 = 105216 B, 9 tiles
    add("fw16_f32_64_128", "f32", 64, 128, F, FWD)
    add("fwd_text_25_mask", "bf16", 64, 25, F, FWD, key_mask=True)
    add("fwd_dropout", "bf16", 64, 197, F, FWD, dropout_p=0.1)

    # ---- masked / dropout backward: head_dim 64 and n <= 256
    add("md_bf16_mask_256", "bf16", 64, 256, B_, BWD_MASKED, key_mask=True)
    add("md_bf16_drop_25", "bf16", 64, 25, B_, BWD_MASKED, dropout_p=0.1)
    add("md_bf16_both_200", "bf16", 64, 200, B_, BWD_MASKED, key_mask=True, dropout_p=0.5)
    add("md_f32_mask_256", "f32", 64, 256, B_, BWD_MASKED, key_mask=True)
    add("md_bf16_mask_257", "bf16", 64, 257, B_, b"key_mask / dropout need head_dim 64 and n <= 256 (got head_dim 64, n 257)",
        key_mask=True)
    add("md_bf16_mask_hd32", "bf16", 32, 25, B_, b"key_mask / dropout need head_dim 64 and n <= 256 (got head_dim 32, n 25)",
        key_mask=True)
    add("md_f32_drop_hd32", "f32", 32, 25, B_, b"key_mask / dropout need head_dim 64", dropout_p=0.1)
    add("md_drop_one", "bf16", 64, 25, B_, b"maeclip_attn_bwd: dropout_p must be < 1", dropout_p=1.0)
    add("md_f32_drop_one", "f32", 64, 40, B_, b"dropout_p must be < 1", key_mask=True, dropout_p=1.0)
    add("md_f32_mask_257_rows", "f32", 64, 257, B_, ROWS, key_mask=True)
    add("md_f32_drop_257_rows", "f32", 64, 257, B_, b"the fp32 long-sequence path has no attention dropout", dropout_p=0.1)

    # ---- fp32: the MFMA kernels while their two images fit, then the rows kernels.
    # hd 32 (144-byte rows): forward 292 npad: 149504 at 512, 168192 at 576; backward 296 npad + 3072: 154624 / 164096
    add("f32_32_fwd_512", "f32", 32, 512, F, FWD16)
    add("f32_32_fwd_513", "f32", 32, 513, F, ROWS)
    add("f32_32_bwd_512", "f32", 32, 512, B_, BWD_FOUR)
    add("f32_32_bwd_513", "f32", 32, 513, B_, ROWS)
    # hd 64 (272-byte rows): forward 548 npad: 140288 at 256, 175360 at 320; backward 552 npad + 6144: 147456 / 165120
    add("f32_64_fwd_256", "f32", 64, 256, F, FWD16)
    add("f32_64_fwd_257", "f32", 64, 257, F, ROWS)
    add("f32_64_bwd_256", "f32", 64, 256, B_, BWD_FOUR)
    add("f32_64_bwd_257", "f32", 64, 257, B_, ROWS)
    add("f32_rows_on_fwd", "f32", 64, 50, F, ROWS, {"ATTN_ROWS": 1})
    add("f32_rows_on_bwd", "f32", 32, 50, B_, ROWS, {"ATTN_ROWS": 1})
    add("bf16_rows_ignored", "bf16", 64, 50, F, FWD, {"ATTN_ROWS": 1})
    add("f32_two_ignored", "f32", 64, 50, B_, BWD_FOUR, {"ATTN_TWO": 1})

    # ---- ATTN_TWO
    add("two_unset_64", "bf16", 64, 50, B_, BWD_OCC)
    add("two_0_64", "bf16", 64, 50, B_, BWD_FOUR, {"ATTN_TWO": 0})
    add("two_1_64", "bf16", 64, 50, B_, BWD_TWO, {"ATTN_TWO": 1})
    add("two_3_64_is_two", "bf16", 64, 50, B_, BWD_TWO, {"ATTN_TWO": 3})
    add("two_1_32", "bf16", 32, 50, B_, BWD_TWO, {"ATTN_TWO": 1, "ATTN_DIAG": 0})
    add("two_3_32", "bf16", 32, 50, B_, BWD_TWO3, {"ATTN_TWO": 3, "ATTN_DIAG": 0})
    add("two_3_32_diag_first", "bf16", 32, 50, B_, BWD_DIAG, {"ATTN_TWO": 3})

    # ---- the fused fp8 copy moves no path, and the rejections hold with it
    add("q8_fwd", "bf16", 64, 197, F, FWD, q8=True)
    add("q8_fwd16", "bf16", 32, 577, F, FWD16, H=4, q8=True)
    add("q8_bwd_diag", "bf16", 64, 197, B_, BWD_DIAG, q8=True)
    add("q8_bwd_two3", "bf16", 32, 50, B_, BWD_TWO3, {"ATTN_TWO": 3, "ATTN_DIAG": 0}, H=4, q8=True)
    add("q8_bwd_16", "bf16", 32, 577, B_, BWD_16, H=4, q8=True)
    add("q8_bwd_occ", "bf16", 64, 50, B_, BWD_OCC, q8=True)
    add("q8_stream", "bf16", 64, 577, F, STREAM, q8=True)
    add("q8_f32_rows", "f32", 64, 300, F, ROWS, q8=True)
    add("q8_lds", "bf16", 64, 700, B_, b"of LDS (> 160 KiB)", {"ATTN_STREAM": 0}, q8=True)
    add("q8_stream_mask", "bf16", 64, 700, F, b"streamed path", key_mask=True, q8=True)
    return c


# ---- tests/test_kernels_gpu.py::test_attention_fwd_bwd: (forward, backward) path per (dtype, mode, shape).
# Every mode pins ATTN_TWO (0 unless "two" / "two3"), ATTN_DIAG, ATTN_BW16 and ATTN_ROWS, so no case is "by
# occupancy". bf16 forward: 16 waves only at (1, 577, 2, 32). "two3" at hd 64 is the two-image kernel; the modes
# skipped there (diag past its LDS, bw16 at <= 8 tiles) have no entry.
def fwd_bwd_paths(dtype, mode, shape):
    B, n, H, hd = shape
    if dtype == "f32":
        if mode == "rows" or n == 577:
            return ROWS, ROWS
        # 16-wave forward: more than 8 tiles and 2 x 548 npad > 160 KiB, which is every hd 64 shape past n = 128
        return (FWD16 if hd == 64 and n > 128 else FWD), BWD_FOUR
    fwd = FWD16 if n == 577 else FWD
    bwd = {"four": BWD_FOUR, "two": BWD_TWO, "two3": BWD_TWO3 if hd == 32 else BWD_TWO, "diag": BWD_DIAG,
           "bw16": BWD_16}[mode]
    return fwd, bwd
