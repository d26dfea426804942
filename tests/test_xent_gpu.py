"""maeclip_xent_fwd / maeclip_xent_bwd against fp64 F.cross_entropy (with
label_smoothing; class-index or class-probability targets) and fp64 autograd on
the CPU, on the fp32 inputs widened to double.

Shapes: M in {1, 2, 5, 65, 257} x C in {1, 2, 3, 5, 64, 65, 257, 1000}, and M in
{1, 2, 5} x C in {B - 1, B, B + 1, 21843} with B = kernels.XENT_REG_COLS, the
forward's register bound (one wave per row up to 256 columns, one workgroup per
row with 1 / 2 / 4 / 8 register pieces up to B, streamed past it). Each with
eps in {0, 0.1}, hard and soft targets, and the logits laid out with row stride
C, round-up-4(C) and C + 12 (an odd stride takes the 4-byte path) plus a base
that is 4 bytes off a 16-byte boundary; the pad columns hold NaN.

Bounds (those of the round-12 loss tests): loss 1e-5 relative; row_loss and lse
1e-5 of max(1, |ref|); dlogits 1e-4 of the row's max |grad| of the reference;
pad columns of dlogits exactly 0; nothing non-finite.

The +-1e4 case keeps its hard labels off the row's arg-max when eps = 0: there
the reference loss and gradient are sums of exp(-gap) terms below 2^-24 of the
unit-size values an fp32 softmax is made of, which no fp32 evaluation resolves
(the row loss would be log1p of a number that rounds to 1)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mae_clip_amd import kernels as K
from tests.helpers import record_parity, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
B_REG = K.XENT_REG_COLS
SHORT_C = (1, 2, 3, 5, 64, 65, 257, 1000)
LONG_C = (B_REG - 1, B_REG, B_REG + 1, 21843)
NAN = float("nan")


@pytest.fixture(autouse=True)
def _device(dev):
    """a GPU test that runs without a GPU is a failure, not a skip (conftest.dev)"""


def rows_of(C):
    return (1, 2, 5, 65, 257) if C <= 1000 else (1, 2, 5)


def up4(n):
    return (n + 3) // 4 * 4


def padded(x, ld, offset=0, fill=NAN):
    """x [M, C] on the device as a view of row stride ld >= C, the pad columns
    (and `offset` floats in front of the base) filled with `fill`"""
    M, C = x.shape
    flat = torch.full((offset + M * ld,), fill, device=DEV, dtype=torch.float32)
    v = flat[offset:].view(M, ld)
    v[:, :C] = x.to(DEV)
    return v


def layouts(C):
    """(name, ld, base offset in floats)"""
    return (("ld=C", C, 0), ("ld=up4", up4(C), 0), ("ld=C+12", C + 12, 0), ("base+4B", up4(C), 1))


def reference(x, labels, Y, eps, scale=1.0):
    """fp64: loss, row terms (their sum is the loss), lse, d loss / d logits"""
    x64 = x.double().requires_grad_(True)
    tgt = labels if Y is None else Y.double()
    rows = F.cross_entropy(x64, tgt, reduction="none", label_smoothing=eps) * (scale / x.shape[0])
    loss = rows.sum()
    (g,) = torch.autograd.grad(loss, x64)
    mean = F.cross_entropy(x64, tgt, label_smoothing=eps) * scale
    assert abs(mean.item() - loss.item()) <= 1e-12 * max(1.0, abs(loss.item()))
    return loss.item(), rows.detach(), torch.logsumexp(x64.detach(), 1), g


def draw(M, C, seed, kind):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, C, generator=g)
    labels = torch.randint(0, C, (M,), generator=g)
    Y = None
    if kind == "soft":
        Y = torch.distributions.Dirichlet(torch.full((C,), 0.5)).sample((M,)).float() if C > 1 else torch.ones(M, 1)
        Y = Y[torch.randperm(M, generator=g)] if M > 1 else Y
    return x, labels, Y


WORST = {}


def compare(tag, x, labels, Y, eps, lay, scale=1.0, ref=None):
    """one forward + backward in layout `lay` against the reference; returns the
    measured deviations (in units of their bounds' scales)"""
    M, C = x.shape
    name, ld, off = lay
    ref = ref or reference(x, labels, Y, eps, scale)
    rloss, rrows, rlse, rg = ref
    xb = padded(x, ld, off)
    yb = None if Y is None else padded(Y, C if ld == C else C + 5, 0)
    lab = None if Y is not None else labels.to(DEV)
    out = K.xent_fwd(xb, lab, yb, C=C, label_smoothing=eps, loss_scale=scale, row_loss=True)
    d = K.xent_bwd(xb, out.lse, lab, yb, C=C, label_smoothing=eps, loss_scale=scale, lse_lo=out.lse_lo)
    loss = out.loss.item()
    row, lse, d = out.row_loss.cpu().double(), out.lse.cpu().double(), d.cpu()
    assert d.shape == (M, ld)
    assert np.isfinite(loss) and torch.isfinite(row).all() and torch.isfinite(lse).all() and torch.isfinite(d).all(), tag
    assert (d[:, C:] == 0).all() and not torch.signbit(d[:, C:]).any(), f"{tag}: pad columns of dlogits"
    e_loss = abs(loss - rloss) / abs(rloss) if rloss != 0 else (0.0 if loss == 0 else float("inf"))
    e_row = ((row - rrows).abs() / rrows.abs().clamp_min(1.0)).max().item()
    e_lse = ((lse - rlse).abs() / rlse.abs().clamp_min(1.0)).max().item()
    gmax = rg.abs().amax(1, keepdim=True)
    gerr = (d[:, :C].double() - rg).abs()
    # a reference row of zeros (C = 1) asks for exact zeros: 0 / 0 -> 0, x / 0 -> inf
    e_g = torch.nan_to_num(gerr / gmax, nan=0.0, posinf=float("inf")).max().item()
    print(f"[xent] {tag} {name}: loss {e_loss:.2e} row {e_row:.2e} lse {e_lse:.2e} grad {e_g:.2e}")
    for k, v in (("loss_rel", e_loss), ("row_loss", e_row), ("lse", e_lse), ("grad_rowmax_rel", e_g)):
        WORST[k] = max(WORST.get(k, 0.0), v)
    assert e_loss <= 1e-5, (tag, name, loss, rloss)
    assert e_row <= 1e-5 and e_lse <= 1e-5, (tag, name, e_row, e_lse)
    assert e_g <= 1e-4, (tag, name, e_g)
    return out, d


@pytest.mark.parametrize("C", SHORT_C + LONG_C)
def test_against_fp64(C):
    WORST.clear()
    for M in rows_of(C):
        for kind in ("hard", "soft"):
            x, labels, Y = draw(M, C, 1000 * M + C, kind)
            for eps in (0.0, 0.1):
                ref = reference(x, labels, Y, eps)
                for lay in layouts(C):
                    compare(f"M{M} C{C} {kind} eps{eps}", x, labels, Y, eps, lay, ref=ref)
    record_parity(f"xent_fp64[C={C}]", **WORST)


def test_soft_rows_that_do_not_sum_to_one():
    WORST.clear()
    for M, C in ((5, 65), (65, 1000), (2, B_REG + 1)):
        x, labels, Y = draw(M, C, 7, "soft")
        Y = Y * torch.linspace(0.25, 3.0, M).view(M, 1)
        Y[0] = 0.0       # a row of no target at all: only the smoothing term is left
        for eps in (0.0, 0.1):
            for lay in layouts(C)[1:3]:
                compare(f"unnormalised M{M} C{C} eps{eps}", x, labels, Y, eps, lay)
    record_parity("xent_soft_unnormalised", **WORST)


def test_rows_spanning_1e4():
    """max-subtraction and the two-float lse: logits spread over +-1e4"""
    WORST.clear()
    for M, C in ((5, 1000), (2, 21843), (5, 64)):
        g = torch.Generator().manual_seed(11)
        x = (torch.rand(M, C, generator=g) * 2 - 1) * 1e4
        top = x.argmax(1)
        x[0, (top[0] + 1) % C] = x[0, top[0]] - 0.5          # a near tie at the top: p ~ (0.62, 0.38)
        off_max = (top + 1 + torch.randint(0, max(C - 1, 1), (M,), generator=g) % (C - 1)) % C
        assert (off_max != top).all()
        Y = torch.distributions.Dirichlet(torch.full((C,), 0.5)).sample((M,)).float()
        for eps in (0.0, 0.1):
            for lay in layouts(C)[:3]:
                compare(f"1e4 M{M} C{C} hard eps{eps}", x, off_max, None, eps, lay)
                compare(f"1e4 M{M} C{C} soft eps{eps}", x, off_max, Y, eps, lay)
        # the label on the arg-max with smoothing: the gradient is O(eps), well resolved
        compare(f"1e4 M{M} C{C} argmax eps0.1", x, top, None, 0.1, layouts(C)[1])
    record_parity("xent_rows_1e4", **WORST)


def np_rank(x, y):
    x = x.numpy()
    out = np.empty(len(y), dtype=np.int64)
    for i, yi in enumerate(y.tolist()):
        j = np.arange(x.shape[1])
        out[i] = int(((x[i] > x[i, yi]) | ((x[i] == x[i, yi]) & (j < yi))).sum())
    return out


@pytest.mark.parametrize("C", (1, 2, 5, 65, 257, 1000, B_REG - 1, B_REG, B_REG + 1, 21843))
@pytest.mark.parametrize("label_dtype", (torch.int64, torch.int32))
def test_rank_breaks_ties_by_index(C, label_dtype):
    M = 5
    g = torch.Generator().manual_seed(C)
    x = (torch.randn(M, C, generator=g) * 2).round() / 2       # steps of 0.5: many exact ties
    labels = torch.randint(0, C, (M,), generator=g)
    x[1] = 0.25                                                # an all-equal row: rank == y
    x[2, labels[2]] = x[2].max()                               # the label ties the maximum
    if C > 2:
        x[2, (labels[2] + 1) % C] = x[2].max()
        x[2, (labels[2] - 1) % C] = x[2].max()
    want = np_rank(x, labels)
    assert want[1] == labels[1].item()
    for lay in layouts(C):
        out = K.xent_fwd(padded(x, lay[1], lay[2]), labels.to(DEV, label_dtype), C=C, want_rank=True)
        assert out.rank.dtype == torch.int32
        assert np.array_equal(out.rank.cpu().numpy().astype(np.int64), want), (lay[0], out.rank.cpu(), want)
    # soft targets: the labels feed the rank alone
    Y = torch.softmax(torch.randn(M, C, generator=g), -1)
    soft = K.xent_fwd(x.to(DEV), labels.to(DEV, label_dtype), Y.to(DEV), want_rank=True)
    assert np.array_equal(soft.rank.cpu().numpy().astype(np.int64), want)
    want_loss = reference(x, labels, Y, 0.0)[0]
    assert abs(soft.loss.item() - want_loss) <= 1e-5 * abs(want_loss)


@pytest.mark.parametrize("C", (5, 257, 1000, B_REG + 1))
@pytest.mark.parametrize("label_dtype", (torch.int64, torch.int32))
def test_invalid_labels(C, label_dtype):
    M = 5
    x, labels, _ = draw(M, C, 3, "hard")
    bad = labels.clone()
    bad[0], bad[2], bad[4] = -1, C, 2 ** 31 - 1
    keep = [1, 3]
    xb = padded(x, up4(C) + 4)
    a = K.xent_fwd(xb, labels.to(DEV, label_dtype), C=C, label_smoothing=0.1, want_rank=True, row_loss=True)
    b = K.xent_fwd(xb, bad.to(DEV, label_dtype), C=C, label_smoothing=0.1, want_rank=True, row_loss=True)
    da = K.xent_bwd(xb, a.lse, labels.to(DEV, label_dtype), C=C, label_smoothing=0.1, lse_lo=a.lse_lo)
    db = K.xent_bwd(xb, b.lse, bad.to(DEV, label_dtype), C=C, label_smoothing=0.1, lse_lo=b.lse_lo)
    assert (b.row_loss[[0, 2, 4]] == 0).all() and (b.rank[[0, 2, 4]] == C).all()
    assert (db[[0, 2, 4]] == 0).all() and torch.isfinite(db).all()
    assert same_bits(b.row_loss[keep], a.row_loss[keep]) and same_bits(db[keep], da[keep])
    assert same_bits(b.lse, a.lse) and torch.equal(b.rank[keep], a.rank[keep])
    # the divisor stays M: the loss is the sum of the kept rows' terms
    want = a.row_loss[keep].double().sum().item()
    assert abs(b.loss.item() - want) <= 1e-6 * abs(want)


@pytest.mark.parametrize("M,C", ((65, 5), (257, 64), (65, 257), (257, 1000), (5, B_REG), (5, B_REG + 1), (2, 21843)))
@pytest.mark.parametrize("kind", ("hard", "soft"))
def test_in_place_repeatable_and_scaled(M, C, kind):
    x, labels, Y = draw(M, C, 5, kind)
    lab = None if kind == "soft" else labels.to(DEV)
    for lay in layouts(C)[1:]:
        xb = padded(x, lay[1], lay[2], fill=0.0)
        yb = None if Y is None else padded(Y, C + 5)
        kw = dict(C=C, label_smoothing=0.1)
        a = K.xent_fwd(xb, lab, yb, row_loss=True, **kw)
        b = K.xent_fwd(xb, lab, yb, row_loss=True, **kw)
        assert same_bits(a.loss, b.loss) and same_bits(a.lse, b.lse) and same_bits(a.row_loss, b.row_loss)
        d = K.xent_bwd(xb, a.lse, lab, yb, lse_lo=a.lse_lo, **kw)
        assert same_bits(d, K.xent_bwd(xb, a.lse, lab, yb, lse_lo=a.lse_lo, **kw)), "two calls"
        # grad_output on the device: a power of two scales every element exactly
        q = K.xent_bwd(xb, a.lse, lab, yb, lse_lo=a.lse_lo, grad_output=torch.full((1,), 0.25, device=DEV), **kw)
        assert same_bits(q, d * 0.25), "grad_output"
        one = K.xent_bwd(xb, a.lse, lab, yb, lse_lo=a.lse_lo, grad_output=torch.ones((), device=DEV), **kw)
        assert same_bits(one, d)
        # in place: dlogits == logits
        xin = xb.clone() if lay[2] == 0 else padded(x, lay[1], lay[2], fill=0.0)
        r = K.xent_bwd(xin, a.lse, lab, yb, lse_lo=a.lse_lo, out=xin, **kw)
        assert r.data_ptr() == xin.data_ptr() and same_bits(xin, d), f"in place, {lay[0]}"


@pytest.mark.parametrize("M,C", ((2, 5), (66, 257), (258, 1000), (4, B_REG + 1)))
@pytest.mark.parametrize("kind", ("hard", "soft"))
def test_half_batches_add_up(M, C, kind):
    """data parallel on two ranks: loss_scale = 1/2 on each half of the batch"""
    x, labels, Y = draw(M, C, 9, kind)
    lab = None if kind == "soft" else labels.to(DEV)
    xb = x.to(DEV)
    yb = None if Y is None else Y.to(DEV)
    kw = dict(label_smoothing=0.1)
    full = K.xent_fwd(xb, lab, yb, **kw)
    dfull = K.xent_bwd(xb, full.lse, lab, yb, lse_lo=full.lse_lo, **kw)
    h = M // 2
    tot, grads = 0.0, []
    for r in (slice(0, h), slice(h, M)):
        lh = None if lab is None else lab[r].contiguous()
        yh = None if yb is None else yb[r]
        o = K.xent_fwd(xb[r], lh, yh, loss_scale=0.5, **kw)
        grads.append(K.xent_bwd(xb[r], o.lse, lh, yh, loss_scale=0.5, lse_lo=o.lse_lo, **kw))
        tot += o.loss.double().item()
    assert abs(tot - full.loss.item()) <= 1e-6 * abs(full.loss.item())
    got = torch.cat(grads).cpu().view(torch.int32).long()
    want = dfull.cpu().view(torch.int32).long()
    assert (got - want).abs().max().item() <= 1, "gradient rows differ by more than 1 ulp"
