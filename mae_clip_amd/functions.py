"""torch.autograd.Functions of the hot path, each a fixed sequence of
libmaeclip kernel launches (no torch compute kernels inside).

Granularity follows the fusion boundaries, not nn.Module boundaries: a whole
pre-LN transformer stack is ONE Function, so the residual-stream gradient, its
bf16 copy and the bias-gradient column partials flow from block to block
inside the backward without extra passes over HBM.

Reference ops replaced (file:line):
  TransformerStackFn  timm Block x depth (modules.py:17-19 -> timm 0.9.12) and
                      HF ViTMAELayer x decoder_depth (modeling_vit_mae.py:455-580)
  PatchTokensFn       timm PatchEmbed + _pos_embed (+ MAE visible-patch gather)
  EncoderHeadFn       timm global_pool="avg" + fc_norm; MAE mae_norm
  DecoderEmbedFn      HF decoder_embed + mask-token unshuffle + pos (:536-566)
  MaeHeadLossFn       HF decoder_norm + decoder_pred + loss (:568-578, :852-859)
  TextStackFn         HF DistilBertModel, trainable (modules.py:34-51 with trainable=True)
  ProjectionHeadFn    modules.py:69-76 (always fp32)
  ClipLossFn          CLIP.py:34-43
  ClassifierHeadFn    timm VisionTransformer.head (nn.Linear, always fp32)
  SoftmaxXentFn       F.cross_entropy(label_smoothing; class-index or probability targets)
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import torch

from . import kernels as K


# --------------------------------------------------------- gradient arena
# Data parallel (mae_clip_amd.distributed.DataParallel) keeps every trainable
# gradient in ONE flat fp32 buffer; the backward of each Function below writes
# a parameter's gradient straight into that parameter's slot, autograd adopts
# the slot as p.grad, and the bucketed all-reduce runs on slices of the flat
# buffer -- no flatten / unflatten copies. Without an arena (single GPU) every
# gradient is a fresh tensor as before.
_ARENA = [None]


def set_grad_arena(arena):
    """Called at the start of every forward: slots are handed out again from here."""
    _ARENA[0] = arena
    if arena is not None:
        arena.begin_forward()


def _arena():
    return _ARENA[0]


def gout(arena, p, shape=None):
    """Output buffer for p's gradient: its arena slot (a fresh view object, so
    autograd's AccumulateGrad adopts it without a copy) when p.grad is None and
    the slot has not been handed out since the forward, else a new tensor
    (gradient accumulation / a second use of p: autograd adds it)."""
    if arena is not None:
        v = arena.slot(p)
        if v is not None:
            return v if shape is None else v.view(shape)
    return torch.empty(shape if shape is not None else p.shape, device=p.device, dtype=torch.float32)


# ------------------------------------------------------------ side stream
_SIDE = {}


def side_stream(device) -> torch.cuda.Stream:
    """One extra HIP stream per device for work that is independent of the
    current stream's chain (weight gradients, the frozen text tower)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    s = _SIDE.get(idx)
    if s is None:
        s = _SIDE[idx] = torch.cuda.Stream(device=idx)
    return s


class WgradQueue:
    """Weight-gradient GEMMs of a transformer stack's backward.

    grouped (default): every dW = dy^T x of the stack is queued and join()
    computes them all in ONE maeclip_wgrad_grouped call on the current stream
    -- one persistent launch whose tiles (4 x layers problems) fill the 256 CUs
    without the fp32 split-K slab round trip that a single 768x3072 or
    512x2048 dW needs to occupy the chip (its inputs stay alive until then).
    Otherwise each dW runs as it becomes ready, on the side stream beside the
    dgrad -> LN -> attention chain (side=True) or inline. Inputs used on the
    side stream get record_stream() so the caching allocator does not hand
    their memory to the current stream while the side stream may still read
    it; join() makes the current stream wait for every queued dW.
    """

    def __init__(self, device, enabled=True, grouped=True):
        self.main = torch.cuda.current_stream(device)
        self.side = side_stream(device) if (enabled and not grouped) else None
        self.grouped = grouped
        self.items = []

    def wgrad(self, dy, x, out=None):
        if self.grouped:
            if out is None:
                out = torch.empty((dy.shape[1], x.shape[1]), device=dy.device, dtype=torch.float32)
            if self.items and self.items[0][0].shape[0] != dy.shape[0]:
                self.flush()
            self.items.append((dy, x, out))
            return out
        if self.side is None:
            return K.linear_wgrad(dy, x, out=out)
        M, N = dy.shape
        if out is None:
            out = torch.empty((N, x.shape[1]), device=dy.device, dtype=torch.float32)
        self.side.wait_stream(self.main)
        with torch.cuda.stream(self.side):
            K.linear_wgrad(dy, x, out=out)
        dy.record_stream(self.side)
        x.record_stream(self.side)
        out.record_stream(self.side)
        return out

    def flush(self):
        if self.items:
            K.wgrad_grouped(self.items)
            self.items = []

    def join(self):
        self.flush()
        if self.side is not None:
            self.main.wait_stream(self.side)


# ---------------------------------------------------------------- stacks
@dataclass
class StackSpec:
    B: int
    n: int
    D: int
    H: int
    eps: float
    dtype: torch.dtype              # compute dtype of GEMM operands / activations
    wT: list                        # per block: (qkv, proj, fc1, fc2) weights in `dtype`
    side: bool = True               # weight gradients on the side stream (when not grouped)
    grouped_wgrad: bool = True      # one grouped launch for all weight gradients of the stack
    w8: list = None                 # fp8 mode: per block ((W, W^T) fp8 operands) x (qkv, proj, fc1, fc2)
    # drop-path (timm DropPath, scale_by_keep) on both residual branches: all off by default
    drop_path: tuple = None         # per block: the drop rate (None / 0: today's launches); not with w8
                                    # (modules.run_stack refuses the pair before anything is launched)
    dp_seed: int = 0
    step_ptr: torch.Tensor = None   # device step counter keying the masks (None: step 0)
    bwd_step_ptr: torch.Tensor = None   # the same step's value as the backward will find it (snapshot slot)
    sample_offset: int = 0          # index of the stack's first sample in the global batch (rank * B)
    block0: int = 0                 # index of the stack's first block in the whole encoder


@dataclass
class DropPath:
    """The draw of one block's two branches for the rows of one launch chain:
    branch key k = 2 * block + (0: attention, 1: MLP) (include/maeclip.h)"""
    p: float
    block: int
    seed: int
    sample_offset: int
    step_ptr: torch.Tensor

    def kw(self, branch):
        return dict(p=self.p, k=2 * self.block + branch, seed=self.seed, sample_offset=self.sample_offset,
                    step_ptr=self.step_ptr)


def drop_rate(spec, i):
    """drop rate of block i of the stack (0: the block does not drop)"""
    return float(spec.drop_path[i]) if spec.drop_path else 0.0


def _drop(spec, i, step_ptr, b0=0):
    """DropPath of block i of the stack for the rows starting at its sample b0
    (None: the block does not drop); step_ptr: the forward's counter, or the
    value the backward reads (step_snapshot)"""
    p = drop_rate(spec, i)
    if p <= 0.0:
        return None
    return DropPath(p, spec.block0 + i, spec.dp_seed, spec.sample_offset + b0, step_ptr)


def _quant8(x, fmt, colsum):
    """fp8 operand of x made by a separate pass (its producer wrote none):
    fp8 blocks, or per-row scales for a launch with column sums (those run on
    the 256-row tile, which has no room for the block scales' LDS images)"""
    return K.quant_rows_fp8(x, fmt) if colsum is not None else K.quant_blocks_fp8(x, fmt)


def _fwd(x, w, w8, xq=None, q8=None, **kw):
    """Forward GEMM of a stack: bf16 / fp32 (w), or fp8 (w8 = (W, W^T)): x in
    e4m3 (xq: already quantised by its producer -- per token by a LayerNorm,
    fp8 blocks by a GEMM epilogue; else a pass here) times W (per output
    channel); q8: an Fp8Blocks the epilogue fills with the output's fp8 copy."""
    if w8 is None:
        return K.linear_fwd(x, w, q8=q8, **kw)
    kw.setdefault("out_dtype", x.dtype)
    xq = xq if xq is not None else _quant8(x, K.FP8_E4M3, kw.get("colsum"))
    return K.linear_fp8(xq, w8[0], q8=q8, **kw)


def _gfmt():
    """fp8 format of the gradient operands (config.fp8_grad_format)"""
    from . import config as CFG
    return K.FP8_E5M2 if getattr(CFG, "fp8_grad_format", "e4m3") == "e5m2" else K.FP8_E4M3


def _dgrad(dy, w, w8, dyq=None, q8=None, **kw):
    """dgrad GEMM dX = dY W: fp8 mode takes dY in config.fp8_grad_format
    (dyq: already quantised by its producer) times W^T (per input channel)."""
    if w8 is None:
        return K.linear_dgrad(dy, w, q8=q8, **kw)
    kw.setdefault("out_dtype", dy.dtype)
    dyq = dyq if dyq is not None else _quant8(dy, _gfmt(), kw.get("colsum"))
    return K.linear_fp8(dyq, w8[1], q8=q8, **kw)


def _b8(f8, M, D, fmt, dev):
    """Fp8Blocks for a GEMM epilogue to fill when its consumer GEMM runs in fp8."""
    return K.new_fp8_blocks(M, D, fmt, dev) if f8 is not None else None


def _attn_q8(f8, M, D, fmt, dev, bwd):
    """Fp8Blocks for the attention to fill (config.fp8_attn_q8), else None (the
    consumer GEMM's operand is then made by a standalone pass)"""
    from . import config as CFG
    return _b8(f8, M, D, fmt, dev) if CFG.fp8_attn_q8[1 if bwd else 0] else None


def _q8(f8, M, D, fmt, dev):
    """Fp8Rows for a LayerNorm to fill when its consumer GEMM runs in fp8."""
    return K.new_fp8_rows(M, D, fmt, dev) if f8 is not None else None


PER_BLOCK = 12  # n1w n1b qkvw qkvb projw projb n2w n2b fc1w fc1b fc2w fc2b


_MB_STREAMS = {}


def mb_stream(device, i):
    """Extra HIP stream i (>= 1) per device for micro-batch i of a stack."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (idx, i)
    s = _MB_STREAMS.get(key)
    if s is None:
        s = _MB_STREAMS[key] = torch.cuda.Stream(device=idx)
    return s


class MicroBatches:
    """The stack's samples cut into S equal micro-batches, each issued on its
    own stream (micro-batch 0 on the current one). A kernel of one
    micro-batch fills the CUs the other's kernel leaves idle in its partial
    last round of tiles and around its launch, so the two chains overlap;
    every kernel still sees whole samples (attention) and whole 64-row groups
    (GEMM column-sum partials), so each micro-batch computes exactly the rows
    the whole-batch launch would (tools/mb_overlap.py: bitwise equal).
    Outputs are row slices of whole-batch buffers, so the grouped weight
    gradients and the column reductions run once on the whole batch."""

    def __init__(self, B, n, S, device):
        self.S = S
        self.Bs = B // S
        self.rows = [(i * self.Bs * n, (i + 1) * self.Bs * n) for i in range(S)]
        self.main = torch.cuda.current_stream(device)
        self.streams = [self.main] + [mb_stream(device, i) for i in range(1, S)]
        # stagger (A/B, MAECLIP_MB_STAGGER=k): micro-batch i > 0 starts a block only
        # after micro-batch i - 1 has issued k launches of it, so that different
        # kernels of the block (GEMM epilogues vs attention / LayerNorm) coincide
        self.stagger = int(os.environ.get("MAECLIP_MB_STAGGER", "0") or 0)
        self._ticks = 0
        self._gate = None

    def tick(self):
        """after each launch of a block: records the stagger gate on the
        micro-batch's stream after its k-th launch"""
        if self.stagger <= 0:
            return
        self._ticks += 1
        if self._ticks == self.stagger:
            self._gate = torch.cuda.Event()
            self._gate.record()

    def fork(self):
        for st in self.streams[1:]:
            st.wait_stream(self.main)

    def join(self):
        for st in self.streams[1:]:
            self.main.wait_stream(st)

    def each(self):
        """(index, row slice, batch slice) under each micro-batch's stream."""
        for i, st in enumerate(self.streams):
            r0, r1 = self.rows[i]
            _MB_ACTIVE[0] = i
            if self._gate is not None:
                st.wait_event(self._gate)
            self._ticks, self._gate = 0, None
            try:
                with torch.cuda.stream(st):
                    yield i, slice(r0, r1), slice(i * self.Bs, (i + 1) * self.Bs)
            finally:
                _MB_ACTIVE[0] = None


_MB_ACTIVE = [None]


def microbatch_active():
    """Index of the micro-batch whose launches are being issued (None outside
    MicroBatches.each): its kernels run concurrently with the other chain's
    (bench.py's launch timer then reports them as overlapped)."""
    return _MB_ACTIVE[0]


def microbatch_count(spec) -> int:
    """Micro-batches for a stack: CFG.stack_microbatches on the bf16 and fp8
    paths (the fp32 parity mode runs one), when every micro-batch keeps whole
    64-row groups of the GEMM column-sum partials (and of the fp8 blocks'
    scale layout)."""
    from . import config as CFG
    S = int(getattr(CFG, "stack_microbatches", 1) or 1)
    # A/B scans only: MAECLIP_MB_D<width> overrides the count for stacks of that width
    S = int(os.environ.get(f"MAECLIP_MB_D{spec.D}", S))
    if S <= 1 or spec.dtype != torch.bfloat16 or spec.B % S:
        return 1
    return S if (spec.B // S * spec.n) % 64 == 0 else 1


def _f8(spec, i):
    """block i's fp8 weight operands ((W, W^T) x (qkv, proj, fc1, fc2)); Nones outside fp8 mode"""
    return spec.w8[i] if spec.w8 is not None else (None,) * 4


def _dst(d, name, shape, dtype, dev):
    """destination `name` of d, else a new tensor (for the outputs a kernel
    wrapper does not allocate itself)"""
    t = d.get(name)
    return t if t is not None else torch.empty(shape, device=dev, dtype=dtype)


def _noop(*a):
    pass


def block_forward(spec, w, p, f8, x, Bs, d={}, tick=_noop, dp=None):
    """The 7 forward launches of one pre-LN block (LN, qkv, attention,
    proj + residual, LN, fc1 + GELU', fc2 + residual) on the rows x [Bs * n, D]
    of Bs whole samples, on the current stream. dp (DropPath, a dropping block):
    9 launches -- proj and fc2 write bias + product alone and a drop-path launch
    each adds the scaled branch to the residual in place. w: the block's (qkv, proj, fc1,
    fc2) weights in spec.dtype, p: its PER_BLOCK parameters, f8: _f8(spec, i).
    d: destinations by name (h1 m1 r1 qkv o lse x1 h2 m2 r2 dgelu a x2), e.g.
    row slices of whole-batch buffers; an output without one is a new tensor.
    tick() is called between launches. Returns (the tensors the backward
    needs, by name; the block's output x2)."""
    wqkv, wproj, w1, w2 = w
    n1w, n1b, _, bqkv, _, bproj, n2w, n2b, _, b1, _, b2 = p
    n, D, H, T = spec.n, spec.D, spec.H, spec.dtype
    hd = D // H
    M, F, dev = Bs * n, w1.shape[0], x.device
    q1 = _q8(f8[0], M, D, K.FP8_E4M3, dev)
    h1, m1, r1, _, _ = K.ln_fwd(x, n1w, n1b, spec.eps, out_dtype=T, q8=q1, y_out=d.get("h1"), mean_out=d.get("m1"),
                                rstd_out=d.get("r1"))
    tick()
    qkv = _fwd(h1, wqkv, f8[0], xq=q1, bias=bqkv, out=d.get("qkv"))
    del q1
    tick()
    o8 = _attn_q8(f8[1], M, D, K.FP8_E4M3, dev, False)   # the proj GEMM's fp8 operand
    o, lse = K.attn_fwd(qkv, Bs, n, H, hd, hd ** -0.5, q8=o8, o_out=d.get("o"), lse_out=d.get("lse"))
    tick()
    if dp is None:
        x1 = _fwd(o, wproj, f8[1], xq=o8, bias=bproj, out_dtype=torch.float32, epilogue=K.EPI_RESID, resid=x,
                  out=d.get("x1"))
    else:
        x1 = _fwd(o, wproj, f8[1], xq=o8, bias=bproj, out_dtype=torch.float32, out=d.get("x1"))
        tick()
        K.droppath_fwd(x, x1, n, **dp.kw(0))
    del o8
    tick()
    q2 = _q8(f8[2], M, D, K.FP8_E4M3, dev)
    h2, m2, r2, _, _ = K.ln_fwd(x1, n2w, n2b, spec.eps, out_dtype=T, q8=q2, y_out=d.get("h2"), mean_out=d.get("m2"),
                                rstd_out=d.get("r2"))
    tick()
    # fc1 epilogue: a = gelu(h), dgelu = gelu'(h) saved for the backward
    # (+ a's fp8 blocks for fc2 in fp8 mode)
    dgelu = _dst(d, "dgelu", (M, F), T, dev)
    a8 = _b8(f8[3], M, F, K.FP8_E4M3, dev)
    a = _fwd(h2, w1, f8[2], xq=q2, q8=a8, bias=b1, epilogue=K.EPI_GELU_D, aux_out=dgelu, out=d.get("a"))
    del q2
    tick()
    if dp is None:
        x2 = _fwd(a, w2, f8[3], xq=a8, bias=b2, out_dtype=torch.float32, epilogue=K.EPI_RESID, resid=x1,
                  out=d.get("x2"))
    else:
        x2 = _fwd(a, w2, f8[3], xq=a8, bias=b2, out_dtype=torch.float32, out=d.get("x2"))
        tick()
        K.droppath_fwd(x1, x2, n, **dp.kw(1))
    return dict(x=x, h1=h1, m1=m1, r1=r1, qkv=qkv, o=o, lse=lse, x1=x1, h2=h2, m2=m2, r2=r2, dgelu=dgelu, a=a), x2


def block_backward(spec, w, p, f8, f8n, t, Bs, d={}, after=_noop, dp=None, below_drops=False):
    """The 7 backward launches of one block (fc2 dgrad x GELU', fc1 dgrad, LN,
    proj dgrad, attention, qkv dgrad, LN) on the rows of Bs whole samples, on
    the current stream. t: the block's tensors of these rows by name -- the
    forward's (block_forward) and the residual-stream gradient from above: g
    (f32), gT (its copy in spec.dtype) and gq (gT's fp8 rows, fp8 mode). The
    outputs are added to t under the names _GRADS books them by; dx, dxT, gq
    and pc1 are the block below's g, gT, gq and column partials. f8n: the fc2
    operand of the block below (its dgrad reads dxT). d: destinations by name;
    after(k) is called between launch k and launch k + 1 (the gradients _GRADS
    lists for launch k can be booked from t there).
    dp (DropPath, a dropping block; its step_ptr holds the forward's step): 9
    launches. The branch gradients are s * g and s * dx1: a drop-path launch in
    front of the fc2 dgrad replaces gT and cpart from above by the scaled copy
    of g and its column partials, and one behind the norm2 backward (part of
    launch 2 for after()) makes dx1T and pc2 from dx1, so _GRADS books the same
    12 gradients from the scaled tensors; the residual path (dres of both
    LayerNorm backwards) stays unscaled. below_drops: the block below makes its
    own fc2 operand, so dxT and pc1 are not produced (None)."""
    wqkv, wproj, w1, w2 = w
    n1w, n2w = p[0], p[6]
    n, D, H = spec.n, spec.D, spec.H
    hd = D // H
    scale = hd ** -0.5
    bf = spec.dtype == torch.bfloat16
    M, F, dev = Bs * n, w1.shape[0], t["g"].device
    gq = t.pop("gq")
    T = spec.dtype
    if dp is not None:
        t["gT"], t["cpart"] = K.droppath_bwd(t["g"], n, dtype=T, out=d.get("gT"), partial=d.get("cpart"), **dp.kw(1))
    # mlp.fc2 (+ GELU backward fused into the dgrad epilogue: dA = (dy W2) * gelu'(h))
    t["dA_part"] = _dst(d, "dA_part", (K.gemm_colsum_rows(M), F), torch.float32, dev)
    dA8 = _b8(f8[2], M, F, _gfmt(), dev)   # fc1's dgrad operand (fp8 mode)
    t["dA"] = _dgrad(t["gT"], w2, f8[3], dyq=gq, q8=dA8, epilogue=K.EPI_MUL_AUX, aux=t["dgelu"], colsum=t["dA_part"],
                     out=d.get("dA"))
    del gq
    after(0)
    # mlp.fc1
    dh2 = _dgrad(t["dA"], w1, f8[2], dyq=dA8, out=d.get("dh2"))
    del dA8
    after(1)
    del t["dA"]
    # norm2 (+ residual gradient)
    q1 = _q8(f8[1], M, D, _gfmt(), dev)
    if dp is None:
        dx1, dx1T, t["pg2"], t["pb2"], t["pc2"] = K.ln_bwd(
            dh2, t["x1"], t["m2"], t["r2"], n2w, dres=t["g"], want_bf16=bf, want_colsum=True, q8=q1,
            dx_out=d.get("dx1"), dxb_out=d.get("dx1T"), pg_out=d.get("pg2"), pb_out=d.get("pb2"), pc_out=d.get("pc2"))
        t["dx1T"] = dx1T if bf else dx1
    else:
        dx1, _, t["pg2"], t["pb2"], _ = K.ln_bwd(dh2, t["x1"], t["m2"], t["r2"], n2w, dres=t["g"], dx_out=d.get("dx1"),
                                                 pg_out=d.get("pg2"), pb_out=d.get("pb2"))
        t["dx1T"], t["pc2"] = K.droppath_bwd(dx1, n, dtype=T, out=d.get("dx1T"), partial=d.get("pc2"), **dp.kw(0))
    after(2)
    # attn.proj
    dO = _dgrad(t["dx1T"], wproj, f8[1], dyq=q1, out=d.get("dO"))
    del q1
    after(3)
    # attention
    dq8 = _attn_q8(f8[0], M, 3 * D, _gfmt(), dev, True)   # the qkv dgrad's fp8 operand
    t["dqkv"], t["qpart"] = K.attn_bwd(t["qkv"], t["o"], dO, t["lse"], Bs, n, H, hd, scale, dqkv_out=d.get("dqkv"),
                                       part_out=d.get("qpart"), q8=dq8)
    del dO
    after(4)
    dh1 = _dgrad(t["dqkv"], wqkv, f8[0], dyq=dq8, out=d.get("dh1"))
    del dq8
    after(5)
    del t["dqkv"]
    # norm1 (+ residual gradient); the fc2 dgrad of the block below reads dxT:
    # quantised here when it is fp8
    t["gq"] = _q8(f8n, M, D, _gfmt(), dev)
    t["dx"], dxT, t["pg1"], t["pb1"], t["pc1"] = K.ln_bwd(
        dh1, t["x"], t["m1"], t["r1"], n1w, dres=dx1, want_bf16=bf and not below_drops, want_colsum=not below_drops,
        q8=t["gq"], dx_out=d.get("dx"), dxb_out=d.get("dxT"), pg_out=d.get("pg1"), pb_out=d.get("pb1"),
        pc_out=d.get("pc1"))
    t["dxT"] = None if below_drops else (dxT if bf else t["dx"])


# The 12 parameter gradients of a block in booking order: (the backward launch
# that completes the inputs, index in the block's parameters, inputs by their
# block_backward names). One input: the column partials of a bias / LayerNorm
# gradient (K.ReduceBatch); two: dy and x of a weight gradient dy^T x
# (WgradQueue). cpart: the column partials of the gradient from above.
_GRADS = ((0, 11, "cpart"), (0, 10, "gT", "a"), (0, 9, "dA_part"), (1, 8, "dA", "h2"), (2, 6, "pg2"), (2, 7, "pb2"),
          (2, 5, "pc2"), (3, 4, "dx1T", "o"), (4, 3, "qpart"), (5, 2, "dqkv", "h1"), (6, 0, "pg1"), (6, 1, "pb1"))


def _book(gi, rb, wq, arena, p, t, launch=None):
    """Queues the gradients of a block's parameters p whose inputs launch
    `launch` of block_backward completed (None: all 12) from the block's
    tensors t; gi: the block's PER_BLOCK slots of the stack's gradient list."""
    for k, j, *names in _GRADS:
        if launch is None or k == launch:
            ins = [t[nm] for nm in names]
            out = gout(arena, p[j])
            gi[j] = (rb.add(ins[0], out=out) if len(ins) == 1 else wq.wgrad(ins[0], ins[1], out=out)).view(p[j].shape)


class TransformerStackFn(torch.autograd.Function):
    """A stack of pre-LN blocks: block_forward / block_backward per block, on
    the whole batch (S = 1: every output a new tensor, each gradient booked as
    its inputs become ready) or on S micro-batches (MicroBatches: row slices
    of whole-batch buffers allocated before the fork, gradients booked on the
    whole batch after the join)."""

    @staticmethod
    def forward(ctx, x, spec: StackSpec, *params):
        B, n, D = spec.B, spec.n, spec.D
        xi = x.reshape(B * n, D)
        S = microbatch_count(spec)
        blocks = [(w, params[i * PER_BLOCK:(i + 1) * PER_BLOCK], _f8(spec, i)) for i, w in enumerate(spec.wT)]
        if S > 1:
            saved, xi = TransformerStackFn._forward_microbatches(spec, blocks, xi, S)
        else:
            saved = []
            for i, (w, p, f8) in enumerate(blocks):
                t, xi = block_forward(spec, w, p, f8, xi, B, dp=_drop(spec, i, spec.step_ptr))
                saved.append(t)
        ctx.saved = saved
        ctx.spec = spec
        ctx.params = params
        ctx.arena = _arena()
        ctx.S = S
        ctx.step_snap = step_snapshot(spec, any(drop_rate(spec, i) > 0 for i in range(len(blocks))))
        return xi.view(B, n, D)

    @staticmethod
    def _forward_microbatches(spec, blocks, xi, S):
        B, n, D, H = spec.B, spec.n, spec.D, spec.H
        M, dev, f32 = B * n, xi.device, torch.float32
        mb = MicroBatches(B, n, S, dev)
        e = lambda shape, dt=spec.dtype: torch.empty(shape, device=dev, dtype=dt)
        # whole-batch buffers allocated on the current stream before the fork;
        # each micro-batch writes its rows on its own stream
        saved = []
        for (_, _, w1, _), _, _ in blocks:
            F = w1.shape[0]
            saved.append(dict(x=None, h1=e((M, D)), m1=e((M,), f32), r1=e((M,), f32), qkv=e((M, 3 * D)), o=e((M, D)),
                              lse=e((B, H, n), f32), x1=e((M, D), f32), h2=e((M, D)), m2=e((M,), f32),
                              r2=e((M,), f32), dgelu=e((M, F)), a=e((M, F))))
        outs = [e((M, D), f32) for _ in blocks]
        mb.fork()
        xin = [xi[r0:r1] for r0, r1 in mb.rows]
        # block by block, each micro-batch's launches on its stream in turn (the
        # captured graph then holds S interleaved chains the replay overlaps)
        for i, (w, p, f8) in enumerate(blocks):
            for mi, rs, bs in mb.each():
                d = {k: v[bs if k == "lse" else rs] for k, v in saved[i].items() if v is not None}
                d["x2"] = outs[i][rs]
                _, xin[mi] = block_forward(spec, w, p, f8, xin[mi], mb.Bs, d, mb.tick,
                                           dp=_drop(spec, i, spec.step_ptr, bs.start))
        mb.join()
        for i in range(len(blocks)):
            saved[i]["x"] = xi if i == 0 else outs[i - 1]
        return saved, outs[-1]

    @staticmethod
    def backward(ctx, gy):
        spec, params, S = ctx.spec, ctx.params, ctx.S
        B, n, D = spec.B, spec.n, spec.D
        bf = spec.dtype == torch.bfloat16
        M, dev = B * n, gy.device
        L = len(spec.wT)
        blocks = [(spec.wT[i], params[i * PER_BLOCK:(i + 1) * PER_BLOCK], _f8(spec, i),
                   _f8(spec, i - 1)[3] if i > 0 else None) for i in range(L)]
        grads = [[None] * PER_BLOCK for _ in range(L)]
        rb = K.ReduceBatch()
        wq = WgradQueue(dev, spec.side, spec.grouped_wgrad)
        g = gy.reshape(M, D)
        if not g.is_contiguous():
            g = g.contiguous()
        # a dropping block makes its fc2 operand and bias partials from g itself
        # (block_backward): the copy from above is then not produced
        drops = [drop_rate(spec, i) > 0 for i in range(L)]
        gT = gq = cpart = None
        if not drops[-1]:
            gT = torch.empty((M, D), device=dev, dtype=torch.bfloat16) if bf else None
            # fp8 copy of gT for the top fc2 dgrad: made with gT here (fp8 mode), then
            # by the LayerNorm backward that produces each next gT
            gq = _q8(blocks[-1][2][3], M, D, _gfmt(), dev)
            cpart = K.rows_colsum(g, out_bf16=gT, q8=gq)
            gT = gT if bf else g
        up = dict(g=g, gT=gT, gq=gq, cpart=cpart)
        del g, gT, gq, cpart
        if S > 1:
            g = TransformerStackFn._backward_microbatches(ctx, blocks, up, rb, wq, grads)
        else:
            for i in reversed(range(L)):
                w, p, f8, f8n = blocks[i]
                t = dict(ctx.saved[i], **up)
                up = None
                block_backward(spec, w, p, f8, f8n, t, B, after=lambda k: _book(grads[i], rb, wq, ctx.arena, p, t, k),
                               dp=_drop(spec, i, ctx.step_snap), below_drops=i > 0 and drops[i - 1])
                _book(grads[i], rb, wq, ctx.arena, p, t, 6)
                ctx.saved[i] = None
                up = dict(g=t["dx"], gT=t["dxT"], gq=t["gq"], cpart=t["pc1"])
                t = None    # the block's remaining tensors go with it
            g = up["g"]
        rb.flush()
        wq.join()
        ctx.saved = None
        return (g.view(B, n, D), None, *(gj for gi in grads for gj in gi))

    @staticmethod
    def _backward_microbatches(ctx, blocks, up, rb, wq, grads):
        spec, S, saved = ctx.spec, ctx.S, ctx.saved
        B, n, D = spec.B, spec.n, spec.D
        M, dev, f32 = B * n, up["g"].device, torch.float32
        mb = MicroBatches(B, n, S, dev)
        e = lambda shape, dt=spec.dtype: torch.empty(shape, device=dev, dtype=dt)
        G = K.ln_bwd_partial_rows(M // S, D)    # LayerNorm partial rows per micro-batch
        GC = K.gemm_colsum_rows(M)              # GEMM column-sum partial rows (64-row groups)
        # whole-batch gradient buffers of every block, written per micro-batch
        bufs = []
        drops = [drop_rate(spec, i) > 0 for i in range(len(blocks))]
        GD = K.droppath_partial_rows(M // S) if any(drops) else 0   # drop-path partial rows per micro-batch
        for i, ((_, _, w1, _), _, _, _) in enumerate(blocks):
            F = w1.shape[0]
            b = dict(dA=e((M, F)), dA_part=e((GC, F), f32), dh2=e((M, D)), dx1=e((M, D), f32),
                     dx1T=e((M, D)), pg2=e((S * G, D), f32), pb2=e((S * G, D), f32),
                     pc2=e((S * G, D), f32), dO=e((M, D)), dqkv=e((M, 3 * D)), qpart=e((B, 3 * D), f32),
                     dh1=e((M, D)), dx=e((M, D), f32), dxT=e((M, D)), pg1=e((S * G, D), f32),
                     pb1=e((S * G, D), f32), pc1=e((S * G, D), f32))
            if drops[i]:    # its own scaled copies of g and dx1, with their partials
                b.update(gT=e((M, D)), cpart=e((S * GD, D), f32), pc2=e((S * GD, D), f32))
            if i > 0 and drops[i - 1]:
                del b["dxT"], b["pc1"]
            bufs.append(b)
        mb.fork()
        # per micro-batch: (f32 residual gradient, its bf16 copy, the copy's fp8
        # rows from the LayerNorm backward that made it -- fp8 mode)
        g, gT, gq = up["g"], up["gT"], up["gq"]
        ups = [dict(g=g[r0:r1], gT=None if gT is None else gT[r0:r1],
                    gq=None if gq is None else K.Fp8Rows(gq.q[r0:r1], gq.s[r0:r1], gq.fmt)) for r0, r1 in mb.rows]
        for i in reversed(range(len(blocks))):
            w, p, f8, f8n = blocks[i]
            for mi, rs, bs in mb.each():
                # a micro-batch's part of each buffer: its rows, its samples (lse, the
                # attention's bias partials), its 64-row groups, its LayerNorm partial rows
                sel = dict.fromkeys(("pg2", "pb2", "pc2", "pg1", "pb1", "pc1"), slice(mi * G, (mi + 1) * G))
                sel.update(lse=bs, qpart=bs, dA_part=slice(rs.start // 64, rs.stop // 64))
                if drops[i]:
                    sel.update(dict.fromkeys(("cpart", "pc2"), slice(mi * GD, (mi + 1) * GD)))
                t = {k: v[sel.get(k, rs)] for k, v in saved[i].items()}
                t.update(ups[mi])
                d = {k: v[sel.get(k, rs)] for k, v in bufs[i].items()}
                block_backward(spec, w, p, f8, f8n, t, mb.Bs, d, after=lambda k: mb.tick(),
                               dp=_drop(spec, i, ctx.step_snap, bs.start), below_drops=i > 0 and drops[i - 1])
                ups[mi] = dict(g=t["dx"], gT=t["dxT"], gq=t["gq"])
        mb.join()
        gT, cpart = up["gT"], up["cpart"]
        for i in reversed(range(len(blocks))):
            # (a dropping block's own gT / cpart in bufs[i] take the place of those from above)
            _book(grads[i], rb, wq, ctx.arena, blocks[i][1], {**saved[i], "gT": gT, "cpart": cpart, **bufs[i]})
            gT, cpart = bufs[i].get("dxT"), bufs[i].get("pc1")
        return bufs[0]["dx"]


# ------------------------------------------------------------ text tower
@dataclass
class TextSpec:
    B: int
    T: int
    D: int
    H: int
    dtype: torch.dtype              # compute dtype of GEMM operands / activations
    wT: list                        # per layer: (q|k|v [3D, D], out_lin, lin1, lin2) weights in `dtype`
    p_drop: float = 0.0             # embeddings / FFN dropout (0 in eval mode)
    p_attn: float = 0.0             # attention-probability dropout
    seed: int = 0
    step_ptr: torch.Tensor = None   # device step counter keying the dropout masks
    bwd_step_ptr: torch.Tensor = None   # the same step's value as the backward will find it (snapshot slot)
    padding_idx: int = 0            # HF: nn.Embedding(vocab, dim, padding_idx=pad_token_id)
    eps: float = 1e-12
    grouped_wgrad: bool = True
    side: bool = True


TEXT_EMB = 4        # word_embeddings, position_embeddings, LayerNorm.weight, LayerNorm.bias
TEXT_PER_LAYER = 16  # (q, k, v, out)_lin.(weight, bias), sa_layer_norm.(w, b), lin1.(w, b), lin2.(w, b), output_layer_norm.(w, b)


def step_snapshot(spec, dropout):
    """The step value a backward redraws its forward's dropout masks from (None
    when no dropout is active): the step counter advances at the end of the
    model's forward, so the backward reads the snapshot slot the counter's
    kernel fills (spec.bwd_step_ptr), else a copy of the counter made now."""
    if spec.step_ptr is None or not dropout:
        return None
    return spec.bwd_step_ptr if spec.bwd_step_ptr is not None else spec.step_ptr.clone()


def text_forward(ids, am, emb, layers, B, T, D, H, dt, p_drop, p_attn, seed, step_ptr, keep, eps=1e-12):
    """The launches of HF DistilBertModel's forward (Embeddings + post-LN
    TransformerBlocks, LN(x + sublayer(x))), shared by the frozen tower
    (modules.DistilBertModel) and TextStackFn. emb: (word, position, LN weight,
    LN bias); layers: per layer (q|k|v weight [3D, D] and bias, out_lin w, b,
    sa_layer_norm w, b, lin1 w, b, lin2 w, b, output_layer_norm w, b), GEMM
    weights in dt. am: the f32 key mask [B, T], or the tokenizer's dense int64
    mask, converted inside the embedding launch. keep: also produce what a
    backward needs (LayerNorm statistics and pre-norm sums, lse, gelu').
    Returns (last_hidden_state rows [B*T, D] f32, f32 key mask, (x, mean, rstd)
    of the embedding LayerNorm, per-layer saved tensors)."""
    hd = D // H
    bf = dt == torch.bfloat16
    f32 = torch.float32
    word, pos, eg, eb = emb
    s0 = seed * 131
    if am.dtype == torch.int64:
        x, am = K.embed_fwd(ids, word, pos, mask=am)
    else:
        x = K.embed_fwd(ids, word, pos)
    h, m0, r0, hT, _ = K.ln_fwd(x, eg, eb, eps, out_dtype=f32, out_dropout=p_drop, seed_out=s0 + 1, want_stats=keep,
                                y2=bf, step_ptr=step_ptr)
    hT = hT if bf else h
    saved = []
    for li, (wqkv, bqkv, wout, bout, sa_w, sa_b, w1, b1, w2, b2, out_w, out_b) in enumerate(layers):
        qkv = K.linear_fwd(hT, wqkv, bqkv)
        o, lse = K.attn_fwd(qkv, B, T, H, hd, hd ** -0.5, key_mask=am, dropout_p=p_attn, seed=s0 + 7 * li + 2,
                            want_lse=keep, step_ptr=step_ptr)
        sa = K.linear_fwd(o, wout, bout, out_dtype=f32)
        a, m1, r1, aT, z1 = K.ln_fwd(sa, sa_w, sa_b, eps, out_dtype=f32, res=h, want_stats=keep, y2=bf, xsum=keep)
        del sa
        aT = aT if bf else a
        # lin1 epilogue: f1 = gelu(.) (+ dgelu = gelu'(.) for a backward)
        dgelu = torch.empty((B * T, w1.shape[0]), device=ids.device, dtype=dt) if keep else None
        f1 = K.linear_fwd(aT, w1, b1, epilogue=K.EPI_GELU_D if keep else K.EPI_GELU, aux_out=dgelu)
        f2 = K.linear_fwd(f1, w2, b2, out_dtype=f32)
        hn, m2, r2, hnT, z2 = K.ln_fwd(f2, out_w, out_b, eps, out_dtype=f32, res=a, in_dropout=p_drop,
                                       seed_in=s0 + 7 * li + 3, want_stats=keep, y2=bf, xsum=keep, step_ptr=step_ptr)
        del f2, a
        if keep:
            saved.append([hT, qkv, o, lse, z1, m1, r1, aT, dgelu, f1, z2, m2, r2])
        h, hT = hn, (hnT if bf else hn)
    return h, am, (x, m0, r0), saved


class TextStackFn(torch.autograd.Function):
    """HF DistilBertModel (modeling_distilbert.py) as one Function:
    last_hidden_state [B, T, D] (f32), by text_forward. The seeds are the
    frozen forward's (modules.DistilBertModel); the backward redraws the three
    kinds of dropout mask (embedding LN output, attention probabilities, FFN
    output) from them and from the forward's step value (step_snapshot)."""

    @staticmethod
    def forward(ctx, ids, am, spec: TextSpec, *params):
        def layers():
            # the q / k / v biases are concatenated as each layer is reached
            for li, (wqkv, wout, w1, w2) in enumerate(spec.wT):
                p = params[TEXT_EMB + li * TEXT_PER_LAYER:TEXT_EMB + (li + 1) * TEXT_PER_LAYER]
                yield (wqkv, torch.cat([p[1], p[3], p[5]]), wout, p[7], p[8], p[9], w1, p[11], w2, p[13], p[14], p[15])

        h, am, emb, ctx.saved = text_forward(ids, am, params[:TEXT_EMB], layers(), spec.B, spec.T, spec.D, spec.H,
                                             spec.dtype, spec.p_drop, spec.p_attn, spec.seed, spec.step_ptr, True,
                                             eps=spec.eps)
        ctx.emb = (ids, am, *emb)
        ctx.spec = spec
        ctx.params = params
        ctx.arena = _arena()
        ctx.step_snap = step_snapshot(spec, spec.p_drop > 0 or spec.p_attn > 0)
        return h.view(spec.B, spec.T, spec.D)

    @staticmethod
    def backward(ctx, gy):
        spec = ctx.spec
        B, T, D, H = spec.B, spec.T, spec.D, spec.H
        hd = D // H
        bf = spec.dtype == torch.bfloat16
        M = B * T
        params = ctx.params
        ar = ctx.arena
        snap = ctx.step_snap
        s0 = spec.seed * 131
        ids, am, x, m0, r0 = ctx.emb
        dev = gy.device
        grads = [None] * len(params)
        rb = K.ReduceBatch()
        wq = WgradQueue(dev, spec.side, spec.grouped_wgrad)
        qkv_bias = []    # (fused q|k|v bias gradient [3D], its three parameters)
        g = gy.reshape(M, D)
        if not g.is_contiguous():
            g = g.contiguous()
        for li in reversed(range(len(spec.wT))):
            wqkv, wout, w1, w2 = spec.wT[li]
            base = TEXT_EMB + li * TEXT_PER_LAYER
            p = params[base:base + TEXT_PER_LAYER]
            hT, qkv, o, lse, z1, m1, r1, aT, dgelu, f1, z2, m2, r2 = ctx.saved[li]
            gi = [None] * TEXT_PER_LAYER
            # output_layer_norm: h' = LN(z2), z2 = dropout(f2) + a
            if spec.p_drop > 0:
                dz2, _, pg, pb, _ = K.ln_bwd(g, z2, m2, r2, p[14])
                df2 = K.dropout(dz2, spec.p_drop, s0 + 7 * li + 3, step_ptr=snap)
                df2T = torch.empty((M, D), device=dev, dtype=torch.bfloat16) if bf else None
                cpart = K.rows_colsum(df2, out_bf16=df2T)
                df2T = df2T if bf else df2
                del df2
            else:
                dz2, df2T, pg, pb, cpart = K.ln_bwd(g, z2, m2, r2, p[14], want_bf16=bf, want_colsum=True)
                df2T = df2T if bf else dz2
            gi[14], gi[15] = rb.add(pg, out=gout(ar, p[14])), rb.add(pb, out=gout(ar, p[15]))
            # ffn.lin2 (+ GELU backward fused into the dgrad epilogue)
            gi[13] = rb.add(cpart, out=gout(ar, p[13]))
            dA_part = torch.empty((K.gemm_colsum_rows(M), w1.shape[0]), device=dev, dtype=torch.float32)
            dA = K.linear_dgrad(df2T, w2, epilogue=K.EPI_MUL_AUX, aux=dgelu, colsum=dA_part)
            gi[12] = wq.wgrad(df2T, f1, out=gout(ar, p[12]))
            del dgelu, f1
            # ffn.lin1; the gradient of a is the FFN's plus the residual's (dz2)
            gi[11] = rb.add(dA_part, out=gout(ar, p[11]))
            da = K.linear_dgrad(dA, w1, out_dtype=torch.float32, epilogue=K.EPI_RESID, resid=dz2)
            gi[10] = wq.wgrad(dA, aT, out=gout(ar, p[10]))
            del dA, dz2
            # sa_layer_norm: a = LN(z1), z1 = out_lin(attention) + h
            dz1, dz1T, pg, pb, pc = K.ln_bwd(da, z1, m1, r1, p[8], want_bf16=bf, want_colsum=True)
            dz1T = dz1T if bf else dz1
            gi[8], gi[9] = rb.add(pg, out=gout(ar, p[8])), rb.add(pb, out=gout(ar, p[9]))
            # attention.out_lin
            gi[7] = rb.add(pc, out=gout(ar, p[7]))
            dO = K.linear_dgrad(dz1T, wout)
            gi[6] = wq.wgrad(dz1T, o, out=gout(ar, p[6]))
            # attention (key mask + the forward's dropout mask redrawn)
            dqkv, qpart = K.attn_bwd(qkv, o, dO, lse, B, T, H, hd, hd ** -0.5, key_mask=am, dropout_p=spec.p_attn,
                                     seed=s0 + 7 * li + 2, step_ptr=snap)
            del dO
            qkv_bias.append((rb.add(qpart), (p[1], p[3], p[5])))
            # q|k|v: one dgrad on the fused weight (+ the residual gradient dz1);
            # the three weight gradients are column slices of dqkv times hT
            g = K.linear_dgrad(dqkv, wqkv, out_dtype=torch.float32, epilogue=K.EPI_RESID, resid=dz1)
            for j in range(3):
                gi[2 * j] = wq.wgrad(dqkv[:, j * D:(j + 1) * D], hT, out=gout(ar, p[2 * j]))
            del dqkv, dz1
            ctx.saved[li] = None
            for j in range(TEXT_PER_LAYER):
                grads[base + j] = gi[j]
        # embeddings: h0 = dropout(LN(word + pos))
        word, pos, eg, eb = params[:TEXT_EMB]
        if spec.p_drop > 0:
            g = K.dropout(g, spec.p_drop, s0 + 1, step_ptr=snap)
        dx, _, pg, pb, _ = K.ln_bwd(g, x, m0, r0, eg)
        grads[2], grads[3] = rb.add(pg, out=gout(ar, eg)), rb.add(pb, out=gout(ar, eb))
        grads[0], grads[1] = K.embed_bwd(dx, ids, word, pos, padding_idx=spec.padding_idx, dword=gout(ar, word),
                                         dpos=gout(ar, pos))
        rb.flush()
        wq.join()
        # the q / k / v bias gradients are the three thirds of the reduced partial
        for li, (b3, ps) in zip(reversed(range(len(spec.wT))), qkv_bias):
            base = TEXT_EMB + li * TEXT_PER_LAYER
            for j, pj in enumerate(ps):
                part = b3[j * D:(j + 1) * D]
                grads[base + 2 * j + 1] = part if ar is None else K.copy_words(part, gout(ar, pj))
        for i, (gr, pr) in enumerate(zip(grads, params)):
            grads[i] = gr.view(pr.shape)
        ctx.saved = None
        ctx.emb = None
        return (None, None, None, *grads)


# ------------------------------------------------------------ patch embed
@dataclass
class PatchSpec:
    B: int
    L: int
    keep: int
    p: int
    kpad: int
    dtype: torch.dtype
    w_T: torch.Tensor        # [D, kpad] patch-embed weight in `dtype`


class PatchTokensFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, ids_shuffle, ids_restore, spec: PatchSpec, w, b, cls, pos):
        Xp = K.patch_gather(img, ids_shuffle, spec.keep, spec.p, spec.kpad, spec.dtype)
        Y = K.linear_fwd(Xp, spec.w_T, b, out_dtype=torch.float32)
        x = K.tokens_fwd(Y, ids_shuffle, pos.view(-1, pos.shape[-1]), cls.view(-1), spec.B, spec.L, spec.keep)
        ctx.save = (Xp, ids_restore)
        ctx.spec = spec
        ctx.wshape = w.shape
        ctx.params = (w, b, cls, pos)
        ctx.arena = _arena()
        return x

    @staticmethod
    def backward(ctx, gx):
        spec = ctx.spec
        Xp, ids_restore = ctx.save
        gx = gx.contiguous()
        w, b, cls, pos = ctx.params
        ar = ctx.arena
        D = pos.shape[-1]
        dY, dpos, dcls = K.tokens_bwd(gx, ids_restore, spec.B, spec.L, spec.keep, spec.dtype,
                                      dpos=gout(ar, pos, (spec.L + 1, D)), dcls=gout(ar, cls, (D,)))
        Kreal = ctx.wshape[1] * ctx.wshape[2] * ctx.wshape[3]
        dWo = gout(ar, w, (ctx.wshape[0], Kreal))
        if Kreal != spec.kpad:
            dWo.copy_(K.linear_wgrad(dY, Xp)[:, :Kreal])
        else:
            K.linear_wgrad(dY, Xp, out=dWo)
        db = K.colsum_reduce(K.rows_colsum(dY), out=gout(ar, b))
        return None, None, None, None, dWo.view(ctx.wshape), db, dcls.view(1, 1, D), dpos.view(1, -1, D)


# ------------------------------------------------------- encoder outputs
class EncoderHeadFn(torch.autograd.Function):
    """features = fc_norm(mean_{t>=1} x[:, t]) ; latent = mae_norm(x) (optional)."""

    @staticmethod
    def forward(ctx, x, latent_dtype, fcn_w, fcn_b, mn_w, mn_b):
        B, n, D = x.shape
        pooled = K.pool_fwd(x)
        feat, fm, fr, _, _ = K.ln_fwd(pooled, fcn_w, fcn_b, 1e-6, out_dtype=torch.float32)
        ctx.mae = mn_w is not None
        latent = None
        if ctx.mae:
            latent, lm, lr, _, _ = K.ln_fwd(x.view(B * n, D), mn_w, mn_b, 1e-6, out_dtype=latent_dtype)
            ctx.lstats = (lm, lr)
        ctx.save = (x, pooled, fm, fr)
        ctx.w = (fcn_w, mn_w)
        ctx.b = (fcn_b, mn_b)
        ctx.arena = _arena()
        if latent is None:
            return feat
        return feat, latent

    @staticmethod
    def backward(ctx, gfeat, glatent=None):
        x, pooled, fm, fr = ctx.save
        fcn_w, mn_w = ctx.w
        B, n, D = x.shape
        dpooled, _, pg, pb, _ = K.ln_bwd(gfeat.contiguous(), pooled, fm, fr, fcn_w)
        fcn_b, mn_b = ctx.b
        ar = ctx.arena
        g_fw, g_fb = K.colsum_reduce(pg, out=gout(ar, fcn_w)), K.colsum_reduce(pb, out=gout(ar, fcn_b))
        g_mw = g_mb = None
        if ctx.mae and glatent is not None:
            # the avg-pool backward rides in the mae_norm LN backward as its
            # residual gradient (no [B, n, D] pool-gradient tensor in HBM)
            lm, lr = ctx.lstats
            dx2, _, pg2, pb2, _ = K.ln_bwd(glatent.contiguous(), x.view(B * n, D), lm, lr, mn_w,
                                           dres_pool=dpooled, pool_n=n)
            dx = dx2.view(B, n, D)
            g_mw, g_mb = K.colsum_reduce(pg2, out=gout(ar, mn_w)), K.colsum_reduce(pb2, out=gout(ar, mn_b))
        else:
            dx = K.pool_bwd(dpooled, n)
        return dx, None, g_fw, g_fb, g_mw, g_mb


# ------------------------------------------------------------ MAE decoder
@dataclass
class DecSpec:
    B: int
    L: int
    keep: int
    dtype: torch.dtype
    w_T: torch.Tensor        # decoder_embed weight in dtype


class DecoderEmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, latent, ids_shuffle, ids_restore, spec: DecSpec, w, b, mask_token, pos):
        y = K.linear_fwd(latent, spec.w_T, b, out_dtype=torch.float32)
        xd = K.unshuffle_fwd(y, ids_restore, mask_token.view(-1), pos.view(-1, pos.shape[-1]), spec.B, spec.L,
                             spec.keep)
        ctx.save = (latent, ids_restore)
        ctx.spec = spec
        ctx.params = (w, b, mask_token)
        ctx.arena = _arena()
        return xd

    @staticmethod
    def backward(ctx, gxd):
        spec = ctx.spec
        latent, ids_restore = ctx.save
        dy, dmask_part, cs = K.unshuffle_bwd(gxd.contiguous(), ids_restore, spec.B, spec.L, spec.keep, spec.dtype)
        w, b, mask_token = ctx.params
        ar = ctx.arena
        dlatent = K.linear_dgrad(dy, spec.w_T)
        dW = K.linear_wgrad(dy, latent, out=gout(ar, w))
        db = K.colsum_reduce(cs, out=gout(ar, b))
        dmask = K.colsum_reduce(dmask_part, out=gout(ar, mask_token, (mask_token.shape[-1],)))
        return dlatent, None, None, None, dW, db, dmask.view(1, 1, -1), None


@dataclass
class MaeHeadSpec:
    p: int
    norm_pix: bool
    mask_count: float
    loss_scale: float
    dtype: torch.dtype
    w_T: torch.Tensor        # decoder_pred weight in dtype, [Npad, Dd] (zero rows past p*p*C)
    b_pad: torch.Tensor = None   # decoder_pred bias padded to Npad (None: no padding)


class MaeHeadLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xd, img, mask, spec: MaeHeadSpec, dn_w, dn_b, wp, bp):
        B, n, Dd = xd.shape
        x2 = xd.view(B * n, Dd)
        h, m, r, _, _ = K.ln_fwd(x2, dn_w, dn_b, 1e-6, out_dtype=spec.dtype)
        pred = K.linear_fwd(h, spec.w_T, bp if spec.b_pad is None else spec.b_pad)
        row = K.mae_loss_fwd(pred, img, mask, spec.p, spec.norm_pix)
        loss = K.colsum_reduce(row.view(-1, 1), scale=1.0 / spec.mask_count).view(())
        ctx.save = (x2, h, m, r, pred, img, mask)
        ctx.spec = spec
        ctx.dn_w = dn_w
        ctx.shape = xd.shape
        ctx.P = wp.shape[0]
        ctx.params = (dn_w, dn_b, wp, bp)
        ctx.arena = _arena()
        return loss

    @staticmethod
    def backward(ctx, gl):
        spec = ctx.spec
        x2, h, m, r, pred, img, mask = ctx.save
        dpred, cs = K.mae_loss_bwd(pred, img, mask, spec.p, spec.norm_pix, gl.contiguous(), spec.mask_count,
                                   spec.loss_scale)
        dn_w, dn_b, wp, bp = ctx.params
        ar = ctx.arena
        dh = K.linear_dgrad(dpred, spec.w_T)
        dWp = gout(ar, wp)
        if dpred.shape[1] != ctx.P:      # padded pred rows (patch 14): slice back
            dWp.copy_(K.linear_wgrad(dpred, h)[:ctx.P])
            dbp = K.colsum_reduce(cs[:, :ctx.P].contiguous() if cs.shape[1] != ctx.P else cs, out=gout(ar, bp))
        else:
            K.linear_wgrad(dpred, h, out=dWp)
            dbp = K.colsum_reduce(cs, out=gout(ar, bp))
        dx, _, pg, pb, _ = K.ln_bwd(dh, x2, m, r, ctx.dn_w)
        return (dx.view(ctx.shape), None, None, None, K.colsum_reduce(pg, out=gout(ar, dn_w)),
                K.colsum_reduce(pb, out=gout(ar, dn_b)), dWp, dbp)


# --------------------------------------------------------- projection head
@dataclass
class ProjSpec:
    p_drop: float
    seed: int
    step_ptr: torch.Tensor = None   # device step counter (dropout mask of the current step)
    bwd_step_ptr: torch.Tensor = None   # the same step's value as the backward will find it (snapshot slot)


class ProjectionHeadFn(torch.autograd.Function):
    """modules.py:69-76 in fp32: z = dropout(fc(gelu(proj(x)))) + proj(x); LN(z)."""

    @staticmethod
    def forward(ctx, x, spec: ProjSpec, wp, bp, wf, bf, lw, lb):
        x = x.contiguous() if x.stride(-1) != 1 else x
        Bn, P = x.shape[0], wp.shape[0]
        pre = torch.empty((Bn, P), device=x.device, dtype=torch.float32)
        g = K.linear_fwd(x, wp, bp, epilogue=K.EPI_GELU, aux_out=pre)
        f = K.linear_fwd(g, wf, bf)
        out, m, r, _, z = K.ln_fwd(f, lw, lb, 1e-5, out_dtype=torch.float32, res=pre, in_dropout=spec.p_drop,
                                   seed_in=spec.seed, xsum=True, step_ptr=spec.step_ptr)
        ctx.save = (x, pre, g, z, m, r)
        ctx.w = (wp, wf, lw)
        ctx.params = (wp, bp, wf, bf, lw, lb)
        ctx.arena = _arena()
        ctx.spec = spec
        ctx.step_snap = step_snapshot(spec, spec.p_drop > 0)
        return out

    @staticmethod
    def backward(ctx, gout_):
        x, pre, g, z, m, r = ctx.save
        wp, wf, lw = ctx.w
        spec = ctx.spec
        wp_, bp_, wf_, bf_, lw_, lb_ = ctx.params
        ar = ctx.arena
        dz, _, pg, pb, _ = K.ln_bwd(gout_.contiguous(), z, m, r, lw)
        df = K.dropout(dz, spec.p_drop, spec.seed, step_ptr=ctx.step_snap) if spec.p_drop > 0 else dz
        dwf = K.linear_wgrad(df, g, out=gout(ar, wf_))
        dbf = K.colsum_reduce(K.rows_colsum(df), out=gout(ar, bf_))
        dpre = K.linear_dgrad(df, wf, out_dtype=torch.float32, epilogue=K.EPI_DGELU, aux=pre, resid=dz)
        dwp = K.linear_wgrad(dpre, x, out=gout(ar, wp_))
        dbp = K.colsum_reduce(K.rows_colsum(dpre), out=gout(ar, bp_))
        dx = K.linear_dgrad(dpre, wp, out_dtype=torch.float32)
        return (dx, None, dwp, dbp, dwf, dbf, K.colsum_reduce(pg, out=gout(ar, lw_)),
                K.colsum_reduce(pb, out=gout(ar, lb_)))


# ------------------------------------------------------------- CLIP loss
def gather_pair(I, T, group):
    """The data-parallel gather of both losses: contiguous (I, T, rows). With a
    group of more than one rank the local [B, P] embeddings of every rank are
    all-gathered in rank order (the global contrastive denominator, SURVEY
    §8e) and rows = (rank * B, B) is the rank's own slice of the gathered
    batch; otherwise the inputs as given and rows = None (all rows)."""
    I, T = I.contiguous(), T.contiguous()
    if group is not None:
        from .distributed import all_gather_rows, world_rank, check_equal_rows
        world, rank = world_rank(group)
        if world > 1:
            B = I.shape[0]
            check_equal_rows(B, group, I.device)
            return all_gather_rows(I, group), all_gather_rows(T, group), (rank * B, B)
    return I, T, None


def _scale_pair_grads(ctx, gl, params):
    """Backward of both loss Functions: ctx.grads = (dI, dT, one scalar gradient
    per parameter of params that is not None, in that order) scaled by the
    device grad_output gl. Returns (dI, dT, one gradient or None per entry of
    params), the scalar gradients in their parameters' arena slots."""
    dI, dT, *scalars = ctx.grads
    ctx.grads = None
    s = gl.reshape(1).contiguous()
    out = [None] * len(params)
    live = [k for k, p in enumerate(params) if p is not None]
    if not live:
        # scaled in place by the device grad_output: one launch, no host sync
        K.scale_by_scalar(s, 1.0, dI, dT, dI, dT)
        return (dI, dT, *out)
    # dI, dT are the halves of one buffer: scaled in place as one tensor, and
    # the first scalar gradient into its parameter's slot in the same launch;
    # a second one in a launch of its own
    both = dI._base.view(-1)
    k = live[0]
    _, out[k] = K.scale_by_scalar(s, 1.0, both, scalars[0], both, gout(ctx.arena, params[k]))
    for k, d in zip(live[1:], scalars[1:]):
        out[k], _ = K.scale_by_scalar(s, 1.0, d, None, gout(ctx.arena, params[k]))
    return (dI, dT, *out)


class ClipLossFn(torch.autograd.Function):
    """CLIP.py:34-43 on the fused fp32 kernel (the gradients come out of the
    same call; the backward only scales them by grad_output).

    group (data parallel, world > 1): gather_pair; every rank evaluates the
    loss of the gathered batch and asks the kernel for the gradient of its own
    B rows only -- so a SUM all-reduce of the parameter gradients is the exact
    global-batch gradient."""

    @staticmethod
    def forward(ctx, I, T, temperature, group=None, log_temperature=None):
        """log_temperature (CLIPModel.log_temperature, f32 [1]): the kernel reads
        tau = exp(theta) from its device memory instead of the float; when it
        requires grad, d loss / d theta comes out of the same call. Under data
        parallelism it is the sum over the rank's own rows, so the SUM
        all-reduce of the parameter gradients needs no rescale."""
        I, T, rows = gather_pair(I, T, group)
        lt = None if log_temperature is None else log_temperature.detach()
        ctx.theta = log_temperature if lt is not None and ctx.needs_input_grad[4] else None
        loss, *ctx.grads = K.clip_loss(I, T, temperature, want_grad=True, grad_rows=rows, log_temperature=lt,
                                       want_dtemp=ctx.theta is not None)
        ctx.arena = _arena()
        return loss

    @staticmethod
    def backward(ctx, gl):
        dI, dT, dth = _scale_pair_grads(ctx, gl, (ctx.theta,))
        return dI, dT, None, None, dth


class ContrastiveLossFn(torch.autograd.Function):
    """InfoNCE / SigLIP on the fused fp32 kernels (K.contrastive_loss), wired as
    ClipLossFn: the same gather and gradient-row slice under data parallelism,
    the gradients out of the forward's call, the backward only scales them by
    grad_output. d theta and d b (sums over the rank's own rows) go into the
    parameters' gradient slots."""

    @staticmethod
    def forward(ctx, I, T, kind, temperature, group=None, log_temperature=None, logit_bias=None):
        I, T, rows = gather_pair(I, T, group)
        lt = None if log_temperature is None else log_temperature.detach()
        lb = None if logit_bias is None else logit_bias.detach()
        ctx.theta = log_temperature if lt is not None and ctx.needs_input_grad[5] else None
        ctx.bias = logit_bias if lb is not None and ctx.needs_input_grad[6] else None
        loss, *ctx.grads = K.contrastive_loss(I, T, kind, temperature, want_grad=True, grad_rows=rows,
                                              log_temperature=lt, logit_bias=lb, want_dtemp=ctx.theta is not None,
                                              want_dbias=ctx.bias is not None)
        ctx.arena = _arena()
        return loss

    @staticmethod
    def backward(ctx, gl):
        dI, dT, dth, db = _scale_pair_grads(ctx, gl, (ctx.theta, ctx.bias))
        return dI, dT, None, None, None, dth, db


class L2NormalizeFn(torch.autograd.Function):
    """y = x / max(||x||, eps) row-wise (F.normalize) on the fp32 kernels."""

    @staticmethod
    def forward(ctx, x, eps=1e-12):
        x = x.contiguous()
        ctx.save_for_backward(x)
        ctx.eps = float(eps)
        return K.l2_normalize(x, eps)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return K.l2_normalize_bwd(x, g.contiguous(), ctx.eps), None


class CombineLossFn(torch.autograd.Function):
    """loss = clip + w * mae on device scalars (one launch; backward: grad_output
    to the CLIP term as is, w * grad_output to the MAE term in one launch)."""

    @staticmethod
    def forward(ctx, clip, mae, w):
        ctx.w = float(w)
        return K.scalar_axpy(clip, mae, w)

    @staticmethod
    def backward(ctx, gl):
        g = gl.reshape(1).contiguous()
        gm, _ = K.scale_by_scalar(g, ctx.w, out_x=torch.empty((), device=g.device, dtype=torch.float32))
        return gl, gm, None


# ------------------------------------------------- classifier head and loss
@dataclass
class HeadSpec:
    C: int                        # classes; the GEMMs run over the padded width w_pad.shape[0]
    w_pad: torch.Tensor           # [Cpad, D] fp32: the head weight, zero rows past C (the parameter when Cpad == C)
    b_pad: torch.Tensor           # [Cpad] fp32 likewise


class ClassifierHeadFn(torch.autograd.Function):
    """logits = feat W^T + b in fp32 (timm's `head`), wired as ProjectionHeadFn.
    The fp32 GEMM wants the class dimension a multiple of 4: it runs on the
    zero-padded copies of spec ([Cpad, D], [Cpad]), the logits are [M, Cpad]
    (columns >= C are zero weight rows: never part of the loss), and dW / db are
    sliced back to the parameters' [C, D] / [C]."""

    @staticmethod
    def forward(ctx, feat, spec: HeadSpec, w, b):
        feat = feat.contiguous()
        ctx.save = (feat,)
        ctx.spec = spec
        ctx.params = (w, b)
        ctx.arena = _arena()
        return K.linear_fwd(feat, spec.w_pad, spec.b_pad)

    @staticmethod
    def backward(ctx, g):
        (feat,) = ctx.save
        spec = ctx.spec
        w, b = ctx.params
        ar = ctx.arena
        g = g.contiguous()
        C, Cpad = spec.C, spec.w_pad.shape[0]
        dfeat = K.linear_dgrad(g, spec.w_pad, out_dtype=torch.float32) if ctx.needs_input_grad[0] else None
        cs = K.rows_colsum(g)
        dW = gout(ar, w)
        if Cpad != C:
            dW.copy_(K.linear_wgrad(g, feat)[:C])
            db = K.colsum_reduce(cs[:, :C].contiguous(), out=gout(ar, b))
        else:
            K.linear_wgrad(g, feat, out=dW)
            db = K.colsum_reduce(cs, out=gout(ar, b))
        return dfeat, None, dW, db


@dataclass
class XentSpec:
    C: int
    label_smoothing: float = 0.0
    loss_scale: float = 1.0       # 1 / world under data parallelism


class SoftmaxXentFn(torch.autograd.Function):
    """loss = loss_scale * F.cross_entropy(logits[:, :C], labels or targets,
    label_smoothing) on the fused fp32 kernel. The backward is one launch: the
    kernel reads grad_output from the device (no host sync, no separate scale
    pass) and zero-fills the pad columns the head's GEMMs run over."""

    @staticmethod
    def forward(ctx, logits, labels, targets, spec: XentSpec):
        out = K.xent_fwd(logits, labels if targets is None else None, targets, C=spec.C,
                         label_smoothing=spec.label_smoothing, loss_scale=spec.loss_scale)
        ctx.save = (logits, labels if targets is None else None, targets, out.lse, out.lse_lo)
        ctx.spec = spec
        return out.loss

    @staticmethod
    def backward(ctx, gl):
        logits, labels, targets, lse, lse_lo = ctx.save
        spec = ctx.spec
        d = K.xent_bwd(logits, lse, labels, targets, C=spec.C, label_smoothing=spec.label_smoothing,
                       loss_scale=spec.loss_scale, grad_output=gl.reshape(1).contiguous(), lse_lo=lse_lo)
        return d, None, None, None
