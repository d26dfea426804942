"""InfoNCE / SigLIP without a GPU: the ABI of the new entry points, the argument
rejections of maeclip_contrastive_loss on the real library (every check comes
before any launch, so the host pointers handed in are never dereferenced on a
device; a call that got past its checks would fail differently, "launch
failed", which is why each case also looks at the message), the O(N) workspace,
the config switch of CLIPModel and a stubbed-launch plumbing run of both kinds.
The kernels are compared with fp64 references in test_contrastive_gpu.py."""
import ctypes

import pytest
import torch

from mae_clip_amd import _lib as L
from tests.helpers import C0, make_batch, product_config
from tests.test_plumbing_cpu import stubbed_kernels

_BUF = (ctypes.c_float * 64)()
P = ctypes.addressof(_BUF) // 16 * 16 + 16      # a 16-byte aligned host address
KW = {k: v for k, v in C0.items() if k != "batch_size"}


@pytest.fixture(scope="module")
def lib():
    return L.load()


def test_abi_and_symbols(lib):
    assert lib.maeclip_abi_version() == 14 and L.ABI_VERSION == 14
    for name, nargs in (("maeclip_contrastive_workspace", 4), ("maeclip_contrastive_loss", 2),
                        ("maeclip_l2_normalize_bwd", 10)):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert len(L._SIGS[name][1]) == nargs, name
    assert L._SIGS["maeclip_contrastive_workspace"][0] is ctypes.c_size_t
    names = [f[0] for f in L.ContrastiveArgs._fields_]
    assert names == ["I", "T", "ld_I", "ld_T", "N", "P", "kind", "temperature", "log_temperature", "logit_bias", "loss",
                     "row_loss_out", "dI", "dT", "ld_dI", "ld_dT", "grad_row0", "grad_rows", "d_log_temperature",
                     "d_logit_bias", "workspace", "ws_bytes"]


def _args(**kw):
    """a valid small call with gradients; kw overrides"""
    d = dict(I=P, T=P, ld_I=64, ld_T=64, N=4, P=64, kind=0, temperature=1.0, loss=P, dI=P, dT=P, ld_dI=64, ld_dT=64,
             grad_row0=0, grad_rows=4, workspace=P, ws_bytes=1 << 20)
    d.update(kw)
    return L.ContrastiveArgs(**d)


CASES = {
    "null args": (None, b"null pointer"),
    "no loss": (dict(loss=None), b"null pointer"),
    "kind 2": (dict(kind=2), b"kind must be 0"),
    "kind -1": (dict(kind=-1), b"kind must be 0"),
    "N 0": (dict(N=0), b"N must be in"),
    "P 96": (dict(P=96), b"P must be 64, 128, 256 or 512"),
    "temperature 0 by value": (dict(temperature=0.0), b"temperature must be > 0"),
    "logit_bias with InfoNCE": (dict(logit_bias=P), b"SigLIP's (kind 1) only"),
    "d_logit_bias with InfoNCE": (dict(d_logit_bias=P), b"SigLIP's (kind 1) only"),
    "d_log_temperature without dI/dT": (dict(dI=None, dT=None, log_temperature=P, d_log_temperature=P),
                                        b"d_log_temperature needs"),
    "d_log_temperature without log_temperature": (dict(d_log_temperature=P), b"d_log_temperature needs"),
    "d_logit_bias without dI/dT": (dict(kind=1, dI=None, dT=None, d_logit_bias=P), b"d_logit_bias needs dI and dT"),
    "dI without dT": (dict(dT=None), b"dI and dT come together"),
    "misaligned log_temperature": (dict(log_temperature=P + 2), b"4-byte aligned"),
    "I not 16-byte aligned": (dict(I=P + 4), b"I/T rows must be 16-byte aligned"),
    "ld_T % 4": (dict(ld_T=66), b"I/T rows must be 16-byte aligned"),
    "ld_I < P": (dict(ld_I=32), b"I/T rows must be 16-byte aligned"),
    "dI not 16-byte aligned": (dict(dI=P + 8), b"dI/dT rows must be 16-byte aligned"),
    "gradient rows past N": (dict(grad_row0=2, grad_rows=3), b"gradient rows out of range"),
    "short workspace": (dict(ws_bytes=64), b"workspace too small or misaligned"),
    "short workspace, SigLIP": (dict(kind=1, ws_bytes=16), b"workspace too small or misaligned"),
    "misaligned workspace": (dict(workspace=P + 4), b"workspace too small or misaligned"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_contrastive_loss_rejects(lib, case):
    kw, what = CASES[case]
    a = None if kw is None else _args(**kw)
    rc = lib.maeclip_contrastive_loss(ctypes.byref(a) if a is not None else None, None)
    msg = lib.maeclip_last_error()
    assert rc == -1, (rc, msg)
    assert what in msg and b"launch failed" not in msg, msg


def test_l2_normalize_bwd_rejects(lib):
    assert lib.maeclip_l2_normalize_bwd(P, P, None, 4, 64, 64, 64, 64, 1e-12, None) == -1
    assert lib.maeclip_l2_normalize_bwd(P, P, P, 4, 64, 32, 64, 64, 1e-12, None) == -1
    assert b"maeclip_l2_normalize_bwd" in lib.maeclip_last_error()
    assert lib.maeclip_l2_normalize_bwd(P, P, P, 0, 64, 64, 64, 64, 1e-12, None) == 0   # no rows: no launch


@pytest.mark.parametrize("kind", [0, 1])
def test_workspace_is_linear_in_n(lib, kind):
    """no N x N matrix: below 1/16 of one at N = 32768, and doubling N no more
    than doubles-and-a-half it"""
    w = lib.maeclip_contrastive_workspace(32768, 256, 4096, kind)
    w2 = lib.maeclip_contrastive_workspace(65536, 256, 4096, kind)
    assert 0 < w < 32768 ** 2 * 4 // 16, w
    assert w < w2 < 2.5 * w, (w, w2)
    assert w % 16 == 0
    # against the soft loss's three matrices at its largest N
    assert lib.maeclip_contrastive_workspace(16384, 256, 2048, kind) * 100 < lib.maeclip_clip_loss_workspace(16384, 256, 2048)


def _model(**over):
    from mae_clip_amd.CLIP import CLIPModel
    with product_config(precision="fp32", side_stream=False, **KW, **over):
        torch.manual_seed(0)
        return CLIPModel()


def test_config_switch_and_state_dict_keys():
    from mae_clip_amd import config as CFG
    assert CFG.clip_loss == "soft" and CFG.normalize_embeddings is True and CFG.logit_bias_init == -10.0
    with pytest.raises(ValueError, match="clip_loss"):
        _model(clip_loss="nonsense")
    soft = set(_model().state_dict())
    assert "logit_bias" not in soft and "log_temperature" not in soft
    assert set(_model(clip_loss="soft").state_dict()) == soft
    assert set(_model(clip_loss="infonce").state_dict()) == soft
    sig = _model(clip_loss="siglip", logit_bias_init=-3.5)
    assert set(sig.state_dict()) == soft | {"logit_bias"}
    assert sig.logit_bias.shape == (1,) and sig.logit_bias.dtype == torch.float32 and sig.logit_bias.item() == -3.5
    assert sig.logit_bias.requires_grad
    lt = _model(clip_loss="infonce", learnable_temperature=True)
    assert set(lt.state_dict()) == soft | {"log_temperature"}


@pytest.mark.parametrize("kind", ["infonce", "siglip", "soft"])
@pytest.mark.parametrize("learnable", [False, True])
def test_training_step_plumbing(monkeypatch, kind, learnable):
    """CLIPModel forward / backward / AdamW with every launch stubbed: the new
    kinds go through maeclip_contrastive_loss (and the normalisation kernels),
    the default through maeclip_clip_loss, never both"""
    from mae_clip_amd.optim import AdamW
    with stubbed_kernels(monkeypatch) as stub:
        m = _model(clip_loss=kind, learnable_temperature=learnable).train()
        opt = AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-3)
        for B in (8, 5):
            opt.zero_grad(set_to_none=True)
            loss = m(make_batch(B, 32))
            assert loss.shape == ()
            loss.backward()
            for n, p in m.named_parameters():
                if p.requires_grad:
                    assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == torch.float32, n
            opt.step()
        new = kind != "soft"
        assert ("maeclip_contrastive_loss" in stub.calls) == new
        assert ("maeclip_clip_loss" in stub.calls) == (not new)
        assert ("maeclip_l2_normalize" in stub.calls) == new and ("maeclip_l2_normalize_bwd" in stub.calls) == new
        assert (m.logit_bias is not None) == (kind == "siglip")
        m.eval()
        with torch.no_grad():
            n0 = stub.calls.count("maeclip_contrastive_loss")
            assert m(make_batch(3, 32)).shape == ()
            assert stub.calls.count("maeclip_contrastive_loss") == n0 + (1 if new else 0)


def test_plumbing_without_normalisation(monkeypatch):
    with stubbed_kernels(monkeypatch) as stub:
        m = _model(clip_loss="siglip", normalize_embeddings=False).train()
        m(make_batch(4, 32)).backward()
        assert "maeclip_contrastive_loss" in stub.calls and "maeclip_l2_normalize" not in stub.calls
        assert m.logit_bias.grad is not None and m.logit_bias.grad.shape == (1,)


def test_kernels_wrapper_argument_checks(monkeypatch):
    from mae_clip_amd import kernels as K
    with stubbed_kernels(monkeypatch):
        I, T = torch.zeros(4, 64), torch.zeros(4, 64)
        one = torch.zeros(1)
        with pytest.raises(ValueError, match="kind"):
            K.contrastive_loss(I, T, "soft", 1.0)
        with pytest.raises(ValueError, match="SigLIP"):
            K.contrastive_loss(I, T, "infonce", 1.0, logit_bias=one)
        with pytest.raises(ValueError, match="want_dtemp"):
            K.contrastive_loss(I, T, "infonce", 1.0, want_dtemp=True)
        with pytest.raises(ValueError, match="want_dbias"):
            K.contrastive_loss(I, T, "infonce", 1.0, want_dbias=True)
        with pytest.raises(ValueError, match="out of range"):
            K.contrastive_loss(I, T, "siglip", 1.0, grad_rows=(2, 3))
        out = K.contrastive_loss(I, T, "siglip", 1.0, log_temperature=one, logit_bias=one, want_dtemp=True,
                                 want_dbias=True, row_loss=True, grad_rows=(1, 2))
        assert [None if t is None else tuple(t.shape) for t in out] == [(), (2, 64), (2, 64), (4,), (1,), (1,)]
        assert out[1]._base is out[2]._base
        assert K.contrastive_loss(I, T, 0, 1.0, want_grad=False)[1:] == (None, None)
