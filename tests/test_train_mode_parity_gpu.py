"""Train-mode parity: WHAT the dropout paths compute, not only that they repeat.

  a. the pooling head       sc_cls_pool_train_fwd / sc_cls_pool_bwd / sc_cls_pool_dz with and without dropout, ragged lengths (T, 1, 0, 37), key splits 1 / default / 64
  b. the layer node         train_hubert.HubertLayersTrainFn, two layers, all four dropout sites (activation dropout included), padded and packed rows
  c. the front-end node     train_front.HubertFrontTrainFn, dropout_input and the dropout on hidden state 0, padded and packed rows
  d. the frozen encoder     FairseqSpeechEncoder_Hubert in train mode (SC_FROZEN_DROPOUT=1), every hidden state, padded and packed rows, d = 128 and d = 768

Every reference is fp64 torch autograd on the CPU (tests/train_mode_ref.py) with the SAME counter-based masks, regenerated on the host by the restatements of
tests/test_dropout_gpu.py.  Metric: per row max|got - ref| / max|ref| for row tensors (outputs, hidden states, dh_in, dz, dx6, xbar, p), max|got - ref| / max|ref|
over the whole tensor for parameter-shaped gradients.  Bound: 4 x MODEL + 1e-3 -- MODEL is the same metric for the CPU model of a correct implementation
(train_mode_ref.py with model=True: the fp64 graph with a rounding node wherever the product stores bf16 / fp32) on exactly these inputs.
`python tools/train_mode_bounds.py` prints every value, checks that the references are well-posed and that every mutant reference (a wrong seed order, site,
stride or rescale) falls outside the bound; `--emit` prints the MODEL dict below.  No literal tolerance appears in this file except the one the older
test_dropout_gpu.py applies to k_b, whose gradient is analytically zero.  The values measured on the MI355X are in profiles/train_mode_parity.txt.

Rows that take no part are judged as the older tests judge them: padded rows (>= lens[b]) are left out of the row metrics; where the product defines them
(p, pp and dz beyond the valid keys, dx6 beyond the valid frames) they must be exactly zero.  An utterance with lens[b] = 0 pools the CLS keys alone: its
probabilities are the softmax over the NQ CLS scores (exactly 1 for NQ = 1) with exact zeros behind them, xbar is the (dropped) mix of the CLS tokens, and its
dz rows and d alpha are exactly zero.

The front-end case (c) feeds the reference the x6 the node itself produced; its MODEL constant comes from the CPU model of the conv stack on the same waves
(the tool has no GPU), a tensor with the same statistics."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import train_mode_ref as R

BF = torch.bfloat16
F64 = torch.float64

# ---- modelled error of a correct implementation per case and tensor: `python tools/train_mode_bounds.py --emit`
MODEL = {
    "pool-768/p0.0/p": 8.99e-08, "pool-768/p0.0/pp": 8.99e-08, "pool-768/p0.0/xbar": 8.19e-08, "pool-768/p0.0/du": 4.49e-08, "pool-768/p0.0/dck": 1.06e-08,
    "pool-768/p0.0/dz": 3.63e-03, "pool-768/p0.0/dalpha": 2.91e-08,
    "pool-768/p0.25/p": 8.99e-08, "pool-768/p0.25/pp": 1.04e-07, "pool-768/p0.25/xbar": 9.19e-08, "pool-768/p0.25/du": 4.15e-08, "pool-768/p0.25/dck": 2.95e-08,
    "pool-768/p0.25/dz": 3.36e-03, "pool-768/p0.25/dalpha": 3.35e-08,
    "pool-cascaded/p0.0/p": 1.79e-07, "pool-cascaded/p0.0/pp": 1.79e-07, "pool-cascaded/p0.0/xbar": 1.09e-07, "pool-cascaded/p0.0/du": 2.96e-08,
    "pool-cascaded/p0.0/dck": 2.94e-08, "pool-cascaded/p0.0/dz": 3.54e-03,
    "pool-cascaded/p0.25/p": 1.79e-07, "pool-cascaded/p0.25/pp": 2.06e-07, "pool-cascaded/p0.25/xbar": 1.04e-07, "pool-cascaded/p0.25/du": 3.06e-08,
    "pool-cascaded/p0.25/dck": 3.29e-08, "pool-cascaded/p0.25/dz": 3.62e-03,
    "pool-large/p0.0/p": 6.13e-08, "pool-large/p0.0/pp": 6.13e-08, "pool-large/p0.0/xbar": 7.53e-08, "pool-large/p0.0/du": 3.20e-08,
    "pool-large/p0.0/dck": 1.60e-08, "pool-large/p0.0/dz": 3.86e-03, "pool-large/p0.0/dalpha": 4.50e-08,
    "pool-large/p0.25/p": 6.13e-08, "pool-large/p0.25/pp": 7.08e-08, "pool-large/p0.25/xbar": 7.62e-08, "pool-large/p0.25/du": 5.38e-08,
    "pool-large/p0.25/dck": 3.58e-08, "pool-large/p0.25/dz": 3.68e-03, "pool-large/p0.25/dalpha": 4.26e-08,
    "pool-192/p0.0/p": 1.23e-07, "pool-192/p0.0/pp": 1.23e-07, "pool-192/p0.0/xbar": 1.03e-07, "pool-192/p0.0/du": 2.78e-08, "pool-192/p0.0/dck": 2.58e-08,
    "pool-192/p0.0/dz": 3.72e-03, "pool-192/p0.0/dalpha": 1.95e-08,
    "pool-192/p0.25/p": 1.23e-07, "pool-192/p0.25/pp": 1.36e-07, "pool-192/p0.25/xbar": 9.81e-08, "pool-192/p0.25/du": 2.76e-08, "pool-192/p0.25/dck": 3.31e-08,
    "pool-192/p0.25/dz": 3.48e-03, "pool-192/p0.25/dalpha": 1.80e-08,
    "node-padded/hidden0": 8.20e-03, "node-padded/hidden1": 1.27e-02, "node-padded/dh_in": 1.09e-02, "node-padded/L0.q_w": 6.66e-03,
    "node-padded/L0.q_b": 5.91e-03, "node-padded/L0.k_w": 6.37e-03, "node-padded/L0.v_w": 6.40e-03, "node-padded/L0.v_b": 6.27e-03, "node-padded/L0.o_w": 5.81e-03,
    "node-padded/L0.o_b": 5.95e-03, "node-padded/L0.ln1_w": 4.24e-03, "node-padded/L0.ln1_b": 4.52e-03, "node-padded/L0.fc1_w": 5.94e-03,
    "node-padded/L0.fc1_b": 5.44e-03, "node-padded/L0.fc2_w": 5.90e-03, "node-padded/L0.fc2_b": 4.32e-03, "node-padded/L0.ln2_w": 4.10e-03,
    "node-padded/L0.ln2_b": 4.06e-03, "node-padded/L1.q_w": 9.51e-03, "node-padded/L1.q_b": 7.01e-03, "node-padded/L1.k_w": 8.70e-03,
    "node-padded/L1.v_w": 5.04e-03, "node-padded/L1.v_b": 4.87e-03, "node-padded/L1.o_w": 5.76e-03, "node-padded/L1.o_b": 5.65e-03,
    "node-padded/L1.ln1_w": 4.96e-03, "node-padded/L1.ln1_b": 5.02e-03, "node-padded/L1.fc1_w": 6.04e-03, "node-padded/L1.fc1_b": 4.58e-03,
    "node-padded/L1.fc2_w": 5.60e-03, "node-padded/L1.fc2_b": 2.94e-03, "node-padded/L1.ln2_w": 3.90e-03, "node-padded/L1.ln2_b": 0.00e+00,
    "node-packed/hidden0": 9.82e-03, "node-packed/hidden1": 1.18e-02, "node-packed/dh_in": 1.23e-02, "node-packed/L0.q_w": 6.72e-03,
    "node-packed/L0.q_b": 5.90e-03, "node-packed/L0.k_w": 8.81e-03, "node-packed/L0.v_w": 6.21e-03, "node-packed/L0.v_b": 5.59e-03, "node-packed/L0.o_w": 6.04e-03,
    "node-packed/L0.o_b": 8.06e-03, "node-packed/L0.ln1_w": 4.20e-03, "node-packed/L0.ln1_b": 4.63e-03, "node-packed/L0.fc1_w": 6.16e-03,
    "node-packed/L0.fc1_b": 7.61e-03, "node-packed/L0.fc2_w": 5.69e-03, "node-packed/L0.fc2_b": 4.77e-03, "node-packed/L0.ln2_w": 5.40e-03,
    "node-packed/L0.ln2_b": 5.34e-03, "node-packed/L1.q_w": 1.16e-02, "node-packed/L1.q_b": 1.15e-02, "node-packed/L1.k_w": 7.25e-03,
    "node-packed/L1.v_w": 5.29e-03, "node-packed/L1.v_b": 4.54e-03, "node-packed/L1.o_w": 7.52e-03, "node-packed/L1.o_b": 4.35e-03,
    "node-packed/L1.ln1_w": 5.41e-03, "node-packed/L1.ln1_b": 4.77e-03, "node-packed/L1.fc1_w": 4.73e-03, "node-packed/L1.fc1_b": 4.47e-03,
    "node-packed/L1.fc2_w": 6.87e-03, "node-packed/L1.fc2_b": 2.63e-03, "node-packed/L1.ln2_w": 3.80e-03, "node-packed/L1.ln2_b": 0.00e+00,
    "node-frozen0/hidden0": 8.29e-03, "node-frozen0/hidden1": 1.16e-02, "node-frozen0/dh_in": 1.29e-02, "node-frozen0/L1.q_w": 9.42e-03,
    "node-frozen0/L1.q_b": 1.10e-02, "node-frozen0/L1.k_w": 8.94e-03, "node-frozen0/L1.v_w": 4.00e-03, "node-frozen0/L1.v_b": 3.86e-03,
    "node-frozen0/L1.o_w": 6.16e-03, "node-frozen0/L1.o_b": 4.59e-03, "node-frozen0/L1.ln1_w": 4.95e-03, "node-frozen0/L1.ln1_b": 3.15e-03,
    "node-frozen0/L1.fc1_w": 6.83e-03, "node-frozen0/L1.fc1_b": 6.78e-03, "node-frozen0/L1.fc2_w": 5.80e-03, "node-frozen0/L1.fc2_b": 3.11e-03,
    "node-frozen0/L1.ln2_w": 4.41e-03, "node-frozen0/L1.ln2_b": 0.00e+00,
    "front-padded/h0": 1.18e-02, "front-padded/dx6": 9.07e-03, "front-padded/flw": 5.92e-03, "front-padded/flb": 5.76e-03, "front-padded/pw": 5.05e-03,
    "front-padded/pb": 4.20e-03, "front-padded/pg": 3.81e-03, "front-padded/pv": 4.80e-03, "front-padded/pbias": 2.89e-03, "front-padded/elw": 4.97e-03,
    "front-padded/elb": 1.87e-03,
    "front-packed/h0": 1.02e-02, "front-packed/dx6": 9.07e-03, "front-packed/flw": 6.65e-03, "front-packed/flb": 4.49e-03, "front-packed/pw": 4.67e-03,
    "front-packed/pb": 4.62e-03, "front-packed/pg": 3.03e-03, "front-packed/pv": 5.18e-03, "front-packed/pbias": 3.10e-03, "front-packed/elw": 6.39e-03,
    "front-packed/elb": 2.11e-03,
    "frozen-tiny3-padded/h0": 1.97e-02, "frozen-tiny3-padded/h1": 1.89e-02, "frozen-tiny3-padded/h2": 1.60e-02, "frozen-tiny3-padded/h3": 1.57e-02,
    "frozen-tiny3-packed/h0": 1.97e-02, "frozen-tiny3-packed/h1": 1.96e-02, "frozen-tiny3-packed/h2": 1.60e-02, "frozen-tiny3-packed/h3": 1.59e-02,
    "frozen-768-padded/h0": 1.25e-02, "frozen-768-padded/h1": 1.33e-02, "frozen-768-padded/h2": 1.62e-02,
    "frozen-768-packed/h0": 1.27e-02, "frozen-768-packed/h1": 1.20e-02, "frozen-768-packed/h2": 1.57e-02,
    "frozen-act-padded/h0": 1.73e-02, "frozen-act-padded/h1": 1.98e-02, "frozen-act-padded/h2": 1.77e-02,
    "frozen-act-packed/h0": 1.73e-02, "frozen-act-packed/h1": 1.80e-02, "frozen-act-packed/h2": 2.09e-02,
}


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _bf(t):
    """values a bf16 tensor can hold, as fp32"""
    return t.to(BF).float()


RESULTS = []          # (key, worst metric, bound): printed by every check


def judge_rows(key, got, ref):
    """Every row of `got` within the bound of MODEL[key]; prints the worst row beside the bound."""
    assert got.shape == ref.shape and got.numel() > 0, (key, got.shape, ref.shape)
    assert torch.isfinite(got.double()).all(), key
    m = R.row_metric(got.double().cpu(), ref)
    worst, bound = m.max().item(), R.bound_of(MODEL[key])
    RESULTS.append((key, worst, bound))
    print(f"{key:44s} worst row {worst:.3e}  model {MODEL[key]:.2e}  bound {bound:.3e}  rows {m.numel()}")
    assert worst <= bound, (key, "row", int(m.flatten().argmax()), "of", m.numel(), "metric", worst, "bound", bound)


def judge_tensor(key, got, ref):
    assert got.shape == ref.shape, (key, got.shape, ref.shape)
    assert torch.isfinite(got.double()).all(), key
    worst, bound = R.tensor_metric(got.double().cpu(), ref), R.bound_of(MODEL[key])
    RESULTS.append((key, worst, bound))
    print(f"{key:44s} tensor    {worst:.3e}  model {MODEL[key]:.2e}  bound {bound:.3e}")
    assert worst <= bound, (key, "metric", worst, "bound", bound)


# ================================================================================================ a. the pooling head
@dataclasses.dataclass(frozen=True)
class PoolCase:
    id: str
    B: int
    T: int
    D: int
    NQ: int
    H: int
    n: int                    # hidden states the frames are mixed from (0: the cascaded form, no mix)
    normalize: bool = False
    f32: bool = False         # dtype of the hidden states

    @property
    def R(self):
        return self.NQ * self.H

    @property
    def lens(self):
        return [self.T, 1, 0, 37][:self.B]          # T, 1, 0 and a value that is no multiple of 4 or 64, as far as B allows


POOL_CASES = (PoolCase("pool-768", 4, 70, 768, 1, 8, 13), PoolCase("pool-cascaded", 3, 37, 128, 8, 1, 0), PoolCase("pool-large", 3, 21, 1024, 1, 8, 25, True, True),
              PoolCase("pool-192", 2, 33, 192, 1, 8, 5))
POOL_P = (0.0, 0.25)
POOL_SEED = 20241
POOL_NSPLIT = (1, None, 64)      # one block per utterance, the default, and more splits than 8-key groups (64 is the entry's maximum; T = 70 has 71 keys)
POOL_TENSORS = ("p", "pp", "xbar", "du", "dck", "dalpha", "dz")


def pool_case(cid):
    return next(c for c in POOL_CASES if c.id == cid)


@functools.lru_cache(maxsize=None)
def pool_inputs(cid):
    c = pool_case(cid)
    g = _g(len(cid) * 1000 + c.T)
    d = dict(hid=None, alpha=None)
    if c.n:
        hid = torch.randn(c.n, c.B, c.T, c.D, generator=g) * 1.5 + 0.2
        d["hid"] = hid if c.f32 else _bf(hid)
        d["alpha"] = torch.softmax(torch.randn(c.n, generator=g), 0).double()
        src = torch.nn.functional.layer_norm(d["hid"].double(), (c.D,)) if c.normalize else d["hid"].double()
        d["x"] = R.r16(torch.einsum("n,nbtd->btd", d["alpha"], src))                # the bf16 store of the mix: what the kernels read
    else:
        d["x"] = R.r16(torch.randn(c.B, c.T, c.D, generator=g).double())
    sd = d["x"].std().item()          # CLS tokens as large as the frames and scores of unit spread: no key of a short utterance holds a negligible probability
    d["cls"] = sd * torch.randn(c.NQ, c.D, generator=g)
    d["u"] = torch.randn(c.R, c.D, generator=g) * c.D ** -0.5 / sd
    d["beta"] = torch.randn(c.R, generator=g)
    d["dzbar"] = torch.randn(c.B, c.R, c.D, generator=g)
    x, cls, u, beta = d["x"], d["cls"].double(), d["u"].double(), d["beta"].double()
    d["scores"] = (x.reshape(c.B * c.T, c.D) @ u.t() + beta).float().contiguous()                  # the kernels' fp32 score inputs, correctly rounded
    d["cls_scores"] = (cls @ u.t() + beta).float().contiguous()
    return d


def pool_keep(c, p, **mut):
    return R.pool_keep(POOL_SEED, c.B, c.R, c.NQ + c.T, c.NQ + c.T, p, **mut)


def pool_reference(cid, p, model=False, keep="product", **mut):
    """-> dict of the POOL_TENSORS (fp64): p, pp [B, R, NQ + T], xbar [B, R, D], du [R, D], dck [NQ, D], dalpha [B, n] | None, dz [B, T, D]"""
    c, d = pool_case(cid), pool_inputs(cid)
    if isinstance(keep, str):
        keep = pool_keep(c, p)
    x = d["x"].clone().requires_grad_(True)
    cls, u = d["cls"].double().requires_grad_(True), d["u"].double().requires_grad_(True)
    alpha = d["alpha"].expand(c.B, c.n).clone().requires_grad_(True) if c.n else None          # one alpha per utterance: d alpha comes out per utterance
    pr, pp, xbar = R.pool_head(x, cls, u, d["beta"].double(), c.lens, c.NQ, c.H, keep, p, d["hid"].double() if c.n else None, alpha, c.normalize, model, **mut)
    got = torch.autograd.grad((xbar * d["dzbar"].double()).sum(), [x, cls, u] + ([alpha] if c.n else []))
    dz, dck, du = got[:3]
    dalpha = got[3] if c.n else None
    return dict(p=pr.detach(), pp=pp.detach(), xbar=xbar.detach(), du=du, dck=dck, dalpha=dalpha, dz=dz)


@functools.lru_cache(maxsize=None)
def pool_reference_cached(cid, p):
    return pool_reference(cid, p)


def _pool_run(c, p, nsplit):
    from speechclip_amd import ops
    d = pool_inputs(c.id)
    dev = torch.device("cuda")
    x_rows = d["x"].to(BF).reshape(c.B * c.T, c.D).to(dev)
    cls, u, dzbar = d["cls"].to(dev).contiguous(), d["u"].to(dev).contiguous(), d["dzbar"].to(dev).contiguous()
    lens_i = torch.tensor(c.lens, dtype=torch.int32, device=dev)
    hid = None
    if c.n:
        hid = (d["hid"] if c.f32 else d["hid"].to(BF)).reshape(c.n, c.B * c.T, c.D).contiguous().to(dev)
    pk, xbar = ops.cls_pool_train_fwd(x_rows, cls, d["scores"].to(dev), d["cls_scores"].to(dev), lens_i, c.B, c.T, c.NQ, c.R, c.D, p, POOL_SEED)
    du, dck, dalpha, ds, pp = ops.cls_pool_bwd(x_rows, cls, hid, pk, dzbar, u, lens_i, c.B, c.T, c.NQ, c.R, c.D, normalize=c.normalize, drop_p=p, seed=POOL_SEED,
                                               nsplit=nsplit, return_ws=True)
    dz = ops.cls_pool_dz(pp, ds, dzbar, u, lens_i, c.B, c.T, c.NQ, c.R, c.D)
    torch.cuda.synchronize()
    return dict(p=pk, pp=pp, xbar=xbar, du=du, dck=dck, dalpha=dalpha, dz=dz.view(c.B, c.T, c.D))


@pytest.mark.gpu
@pytest.mark.parametrize("p", POOL_P)
@pytest.mark.parametrize("cid", [c.id for c in POOL_CASES])
def test_pooling_head_forward_and_backward_against_fp64_with_the_host_mask(cid, p):
    c = pool_case(cid)
    ref = pool_reference_cached(cid, p)
    keep = pool_keep(c, p)
    K = c.NQ + c.T
    key = lambda t: f"{cid}/p{p}/{t}"      # noqa: E731
    for nsplit in POOL_NSPLIT:
        got = _pool_run(c, p, nsplit)
        S = got["du"].shape[0] // c.B
        assert got["du"].shape == (c.B * S, c.R, c.D) and got["dck"].shape == (c.B * S, c.NQ, c.D)
        print(f"-- {cid} p={p} nsplit={nsplit} (S={S})")
        pk, pp = got["p"].cpu(), got["pp"].cpu()
        for b, n in enumerate(c.lens):
            assert bool((pk[b, :, c.NQ + n:] == 0).all()) and bool((pp[b, :, c.NQ + n:] == 0).all()), (b, "p / pp beyond the valid keys")
            if n == 0 and c.NQ == 1:
                assert bool((pk[b, :, 0] == 1.0).all()), "an utterance without frames: the one CLS key holds all the probability"
        # the mask restated: pp is p times keep / (1 - p), one fp32 product of the kernel's own p and the fp32 rescale
        scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
        want = pk if keep is None else pk * keep * float(scale)
        assert torch.equal(pp, want), (cid, p, "pp != p * keep / (1 - p)", int((pp != want).sum()))
        judge_rows(key("p"), pk, ref["p"])
        judge_rows(key("pp"), pp, ref["pp"])
        judge_rows(key("xbar"), got["xbar"], ref["xbar"])
        judge_tensor(key("du"), got["du"].view(c.B, S, c.R, c.D).sum((0, 1)), ref["du"])
        judge_tensor(key("dck"), got["dck"].view(c.B, S, c.NQ, c.D).sum((0, 1)), ref["dck"])
        if c.n:
            da = got["dalpha"].view(c.B, S, c.n).sum(1).cpu()
            judge_tensor(key("dalpha"), da, ref["dalpha"])
        else:
            assert got["dalpha"] is None
        dz = got["dz"].cpu()
        for b, n in enumerate(c.lens):
            assert bool((dz[b, n:] == 0).all()), (b, "dz beyond the valid frames")
            if n == 0 and c.n:
                assert bool((got["dalpha"].view(c.B, S, c.n)[b] == 0).all()), "an utterance without frames has no d alpha"
        rows = torch.cat([dz[b, :n] for b, n in enumerate(c.lens)])
        judge_rows(key("dz"), rows, torch.cat([ref["dz"][b, :n] for b, n in enumerate(c.lens)]))


# ================================================================================================ b. the layer node
@dataclasses.dataclass(frozen=True)
class NodeCase:
    id: str
    rows: tuple               # rows per utterance in the layout
    lens: tuple               # valid keys per utterance
    packed: bool
    train: tuple

    @property
    def B(self):
        return len(self.rows)

    @property
    def offsets(self):
        off = [0]
        for r in self.rows:
            off.append(off[-1] + r)
        return off


NODE_CASES = (NodeCase("node-padded", (70, 70, 70), (70, 64, 33), False, (True, True)), NodeCase("node-packed", (70, 65, 2, 1), (70, 65, 2, 1), True, (True, True)),
              NodeCase("node-frozen0", (70, 70, 70), (70, 64, 33), False, (False, True)))
NODE_D, NODE_H, NODE_FFN, NODE_LAYERS = 128, 2, 256, 2
NODE_RATES = dict(hidden=0.1, attention=0.1, activation=0.1)
NODE_SEED = 987654


def node_case(cid):
    return next(c for c in NODE_CASES if c.id == cid)


def node_layout(c):
    return dict(row_off=c.offsets, Tmax=max(c.rows)) if c.packed else dict(B=c.B, Tp=c.rows[0])


@functools.lru_cache(maxsize=None)
def node_inputs(cid):
    """16 tensors per layer (matrices hold bf16 values: the product's 16-bit operand copy is then exact), h_in and the gradient of both hidden states (bf16 values,
    zero on the rows >= lens[b]: nothing flows back from padded frames)."""
    c = node_case(cid)
    d, ffn = NODE_D, NODE_FFN
    g = _g(40 + len(cid))
    shapes = [(d, d), (d,), (d, d), (d,), (d, d), (d,), (d, d), (d,), (d,), (d,), (ffn, d), (ffn,), (d, ffn), (d,), (d,), (d,)]
    layers = []
    for _ in range(NODE_LAYERS):
        ps = []
        for i, sh in enumerate(shapes):
            t = _bf(0.08 * torch.randn(*sh, generator=g)) if len(sh) == 2 else 0.05 * torch.randn(*sh, generator=g)
            ps.append(1.0 + t if i in (8, 14) else t)
        layers.append(ps)
    M = c.offsets[-1]
    h_in = _bf(torch.randn(M, d, generator=g))
    dh = _bf(torch.randn(NODE_LAYERS, M, d, generator=g))
    for b, n in enumerate(c.lens):
        dh[:, c.offsets[b] + n:c.offsets[b + 1]] = 0
    return dict(layers=layers, h_in=h_in, dh=dh)


def node_masks(c, plan=None, attn_kw=None, rescale_off=None):
    """masks[li][b] for the rows of utterance b.  plan(li, seeds) -> the layer's (sa, s1, s2, s3), default seeds[4 li : 4 li + 4].
    MUTANTS: another plan, attn_kw (b -> keywords of train_mode_ref.attn_mask), rescale_off = (li, site): that site's mask without its 1 / (1 - p)."""
    seeds = R.site_seeds(NODE_SEED, 4 * NODE_LAYERS + 4)
    lay = node_layout(c)
    out = []
    for li in range(NODE_LAYERS):
        s4 = seeds[4 * li:4 * li + 4] if plan is None else plan(li, seeds)
        per = []
        for b in range(c.B):
            m = R.layer_masks(s4, lay, b, c.rows[b], NODE_D, NODE_FFN, NODE_H, NODE_RATES, **(attn_kw(b) if callable(attn_kw) else (attn_kw or {})))
            if rescale_off is not None and rescale_off[0] == li:
                m[rescale_off[1]] = m[rescale_off[1]] * (1 - NODE_RATES["attention" if rescale_off[1] == "attn" else "activation" if rescale_off[1] == "d2" else "hidden"])
            per.append(m)
        out.append(per)
    return out


def node_reference(cid, model=False, masks=None, bwd_masks=None, wiring=()):
    c, d = node_case(cid), node_inputs(cid)
    off = c.offsets
    xs = [d["h_in"][off[b]:off[b + 1]].double() for b in range(c.B)]
    dh = [[d["dh"][li, off[b]:off[b + 1]].double() for b in range(c.B)] for li in range(NODE_LAYERS)]
    layers = [[p.double() for p in lp] for lp in d["layers"]]
    return R.layer_node(xs, layers, list(c.lens), masks or node_masks(c), dh, c.train, model, bwd_masks, wiring)


@functools.lru_cache(maxsize=None)
def node_reference_cached(cid):
    return node_reference(cid)


def node_rows(c, per_utt):
    """the judged rows: rows < lens[b] of every utterance, concatenated"""
    return torch.cat([t[:n] for t, n in zip(per_utt, c.lens)])


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c.id for c in NODE_CASES])
def test_layer_node_with_all_four_dropouts_against_fp64_with_the_host_masks(cid):
    from speechclip_amd.train_hubert import HubertLayersTrainFn
    c, d = node_case(cid), node_inputs(cid)
    ref = node_reference_cached(cid)
    dev = torch.device("cuda")
    off, M = c.offsets, c.offsets[-1]
    params = [p.clone().to(dev).requires_grad_(True) for lp in d["layers"] for p in lp]
    h_in = d["h_in"].to(BF).to(dev).requires_grad_(True)
    meta = dict(B=c.B, Tp=max(c.rows), H=NODE_H, eps=1e-5, train=list(c.train), drop=dict(NODE_RATES, seed=NODE_SEED))
    if c.packed:
        meta["pack"] = dict(row_off=off, rows_max=max(c.rows), total=M)
    hidden = HubertLayersTrainFn.apply(meta, h_in, torch.tensor(c.lens, dtype=torch.int32, device=dev), *params)
    hidden.backward(d["dh"].to(BF).to(dev))
    torch.cuda.synchronize()
    assert hidden.shape == (NODE_LAYERS, M, NODE_D)
    split = lambda t: [t[off[b]:off[b + 1]].float().cpu() for b in range(c.B)]      # noqa: E731
    for li in range(NODE_LAYERS):
        judge_rows(f"{cid}/hidden{li}", node_rows(c, split(hidden[li].detach())), node_rows(c, ref["hidden"][li]))
    judge_rows(f"{cid}/dh_in", node_rows(c, split(h_in.grad)), node_rows(c, ref["dh_in"]))
    for li in range(NODE_LAYERS):
        mine = params[16 * li:16 * li + 16]
        if not c.train[li]:
            assert all(p.grad is None for p in mine), "an untrained layer has no parameter gradients"
            continue
        for name, p, r in zip(R.LAYER_NAMES, mine, ref["grads"][li]):
            if name == "k_b":      # exactly zero in theory (softmax rows are shift invariant): as test_dropout_gpu.py judges it
                assert p.grad.float().norm().item() < 1e-2 * mine[0].grad.float().norm().item(), (li, name)
                continue
            judge_tensor(f"{cid}/L{li}.{name}", p.grad.float(), r)


# ================================================================================================ c. the front-end node
FRONT_LENS = (4000, 2500, 3300)
FRONT_DROP = dict(features=0.25, hidden=0.1, seed=24680)
FRONT_GRAD_MULT = 0.1
FRONT_LAYOUTS = ("padded", "packed")
FRONT_GRADS = ("flw", "flb", "pw", "pb", "pg", "pv", "pbias", "elw", "elb")          # front_params()[9:18]: feature LayerNorm, projection, positional conv, encoder LayerNorm


def _tiny_hubert(seed, **over):
    """module.hubert.HubertModel on the CPU: the tiny default-extractor config with non-trivial norm affines and biases."""
    from oracle.hubert_ref import HubertRefConfig, randomize_norm_affine
    from speechclip_amd.module.hubert import HubertConfig, HubertModel
    ref_fields = {k: over.pop(k) for k in list(over) if k in {f.name for f in dataclasses.fields(HubertRefConfig)}}
    cfg = HubertConfig(**dataclasses.asdict(dataclasses.replace(HubertRefConfig.tiny(), **ref_fields)), **over)
    torch.manual_seed(seed)
    enc = HubertModel(cfg)
    randomize_norm_affine(enc, _g(seed + 1))
    with torch.no_grad():          # layer branches as large as the residual they join (the 0.02 init hides a wrong branch mask), a positional conv that matters, weight_g away from |v|
        for lyr in enc.encoder.layers:
            for m in lyr.modules():
                if isinstance(m, torch.nn.Linear):
                    m.weight.mul_(4.0 * (128.0 / cfg.encoder_embed_dim) ** 0.5)
        pc = getattr(enc.encoder.pos_conv, "0")
        pc.weight_v.mul_(3.0)
        pc.weight_g.copy_(pc.weight_v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt() * (1.0 + 0.1 * torch.randn(pc.weight_g.shape, generator=_g(seed + 2))))
        pc.bias.add_(0.05 * torch.randn(pc.bias.shape, generator=_g(seed + 3)))
    return enc


def _waves(lens, seed):
    g = _g(seed)
    wav = torch.zeros(len(lens), max(lens))
    for b, l in enumerate(lens):
        wav[b, :l] = 0.3 * torch.randn(l, generator=g)
    return wav


@functools.lru_cache(maxsize=None)
def front_setup():
    """(enc on the CPU, wav, geometry per layout, dh0 per utterance [valid_b, d] of bf16 values)"""
    enc = _tiny_hubert(21)
    wav = _waves(FRONT_LENS, 22)
    L = wav.shape[1]
    T0, T, P0, Tp = enc.frame_geometry(L)
    valid = enc.valid_frames(FRONT_LENS, L, T)
    pack = enc.packed_geometry(FRONT_LENS, L, need_rows=[min(round(l / 320), T) for l in FRONT_LENS])
    geo = dict(T0=T0, T=T, P0=P0, Tp=Tp, valid=valid, pack=pack,
               layout=dict(padded=dict(B=len(FRONT_LENS), Tp=Tp), packed=dict(row_off=pack["row_off"], Tmax=pack["rows_max"])))
    g = _g(23)
    dh0 = [_bf(torch.randn(v, enc.cfg.encoder_embed_dim, generator=g)).double() for v in valid]
    return enc, wav, geo, dh0


def front_x6_model():
    """The tool's stand-in for the node's x6: the CPU model of the conv stack on the same waves (bf16 values), the valid rows of every utterance."""
    enc, wav, geo, _ = front_setup()
    return [R.conv_stack(enc, wav[b], FRONT_LENS[b], model=True)[:geo["valid"][b]] for b in range(len(FRONT_LENS))]


def front_masks(layout, b, n, swap=False, rescale=True):
    enc, _, geo, _ = front_setup()
    sf, sh = FRONT_DROP["seed"] ^ R.FRONT_FEATURES_XOR, FRONT_DROP["seed"] ^ R.FRONT_HIDDEN_XOR
    if swap:
        sf, sh = sh, sf
    return R.front_masks(sf, sh, geo["layout"][layout], b, n, enc.cfg.encoder_embed_dim, FRONT_DROP, rescale)


def front_reference(layout, x6, model=False, masks=None, bwd_masks=None):
    """x6[b] fp64 [valid_b, C] -> dict(h0[b], dx6[b], grads: name -> tensor)"""
    enc, _, geo, dh0 = front_setup()
    P = {k: v.clone().requires_grad_(True) for k, v in R.front_params_of(enc).items()}
    leaves = [x.detach().clone().requires_grad_(True) for x in x6]
    loss, h0s = 0.0, []
    for b, x in enumerate(leaves):
        n = geo["valid"][b]
        m = masks[b] if masks is not None else front_masks(layout, b, n)
        h0 = R.front_stretch(x, n, P, m, enc.cfg.conv_pos_groups, enc.cfg.conv_pos, model, FRONT_GRAD_MULT, None if bwd_masks is None else bwd_masks[b])
        h0s.append(h0.detach())
        loss = loss + (h0 * dh0[b]).sum()
    got = torch.autograd.grad(loss, leaves + [P[k] for k in FRONT_GRADS])
    return dict(h0=h0s, dx6=list(got[:len(x6)]), grads=dict(zip(FRONT_GRADS, got[len(x6):])))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", FRONT_LAYOUTS)
def test_front_end_node_dropouts_against_fp64_with_the_host_masks(layout, monkeypatch):
    from speechclip_amd import ops, train_front
    from speechclip_amd.train_front import HubertFrontTrainFn, front_params
    enc_cpu, wav, geo, dh0 = front_setup()
    import copy
    enc = copy.deepcopy(enc_cpu).cuda()
    cfg = enc.cfg
    dev = torch.device("cuda")
    B, d, Tp, valid = len(FRONT_LENS), cfg.encoder_embed_dim, geo["Tp"], geo["valid"]
    packed = layout == "packed"
    off = geo["pack"]["row_off"] if packed else [b * Tp for b in range(B + 1)]
    M = off[-1]
    meta = dict(conv_layers=[tuple(c) for c in cfg.conv_layers], T0=geo["T0"], P0=geo["P0"], Tp=Tp, d=d, G=cfg.conv_pos_groups, Kw=cfg.conv_pos,
                grad_mult=FRONT_GRAD_MULT, normalize=bool(cfg.normalize), drop=dict(FRONT_DROP))
    if packed:
        pk = geo["pack"]
        meta["pack"] = dict(row_off=ops.dev_ints(pk["row_off"], torch.int32, dev), rows_max=pk["rows_max"], total=pk["total"], scale0=pk["scale0"])
    seen = {}
    tail_backward = train_front._tail_backward

    def spy(lay, meta_, ds, u, xp, feats, x6, *rest):          # observes the node's own x6 and the gradient it hands to the conv stack; changes nothing
        out = tail_backward(lay, meta_, ds, u, xp, feats, x6, *rest)
        seen["x6"], seen["dx6"] = x6.detach().clone(), out[0].detach().clone()
        return out
    monkeypatch.setattr(train_front, "_tail_backward", spy)
    prm = front_params(enc)
    for p in prm:
        p.requires_grad_(True)
    h0 = HubertFrontTrainFn.apply(meta, wav.to(dev), ops.dev_ints(valid, torch.int32, dev), *prm)
    assert h0.shape == (M, d)
    dh = torch.zeros(M, d)
    for b in range(B):
        dh[off[b]:off[b] + valid[b]] = dh0[b].float()
    h0.backward(dh.to(BF).to(dev))
    torch.cuda.synchronize()
    x6 = [seen["x6"][off[b]:off[b] + valid[b]].double().cpu() for b in range(B)]
    ref = front_reference(layout, x6)
    cat = lambda ts: torch.cat(list(ts))      # noqa: E731
    judge_rows(f"front-{layout}/h0", cat(h0.detach()[off[b]:off[b] + valid[b]].float().cpu() for b in range(B)), cat(ref["h0"]))
    dx6 = seen["dx6"].float().cpu()
    judge_rows(f"front-{layout}/dx6", cat(dx6[off[b]:off[b] + valid[b]] for b in range(B)), cat(ref["dx6"]))
    for b in range(B):
        assert bool((dx6[off[b] + valid[b]:off[b + 1]] == 0).all()), (b, "dx6 beyond the valid frames")
    for name, p in zip(FRONT_GRADS, prm[9:18]):
        judge_tensor(f"front-{layout}/{name}", p.grad.float(), ref["grads"][name].reshape(p.shape))


# ================================================================================================ d. the frozen encoder in train mode
@dataclasses.dataclass(frozen=True)
class FrozenCase:
    id: str
    lens: tuple
    over: tuple               # config overrides (name, value)


FROZEN_CASES = (FrozenCase("frozen-tiny3", (8000, 6000, 3000), (("encoder_layers", 3),)),
                FrozenCase("frozen-768", (4800, 3000, 4100), (("encoder_embed_dim", 768), ("encoder_attention_heads", 12), ("encoder_ffn_embed_dim", 1536), ("conv_pos_groups", 16))),
                FrozenCase("frozen-act", (5000, 2600), (("activation_dropout", 0.1),)))
FROZEN_TORCH_SEED = 5


def frozen_case(cid):
    return next(c for c in FROZEN_CASES if c.id == cid)


def frozen_module(cid):
    """A fresh FairseqSpeechEncoder_Hubert on the CPU, deterministic per case."""
    from speechclip_amd.module import FairseqSpeechEncoder_Hubert
    c = frozen_case(cid)
    hc = _tiny_hubert(31 + len(cid), **dict(c.over)).cfg
    torch.manual_seed(32 + len(cid))
    mod = FairseqSpeechEncoder_Hubert("hubert", feat_select_idx="hidden_states", max_audio_len=100000, hubert_config=hc)
    mod.encoder.load_state_dict(_tiny_hubert(31 + len(cid), **dict(c.over)).state_dict())
    return mod


def frozen_seed():
    """The seed the module draws in its forward after torch.manual_seed(FROZEN_TORCH_SEED): one torch.randint(0, 2^31 - 1) from the default generator."""
    state = torch.random.get_rng_state()
    torch.manual_seed(FROZEN_TORCH_SEED)
    seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    torch.random.set_rng_state(state)
    return seed


@functools.lru_cache(maxsize=None)
def frozen_setup(cid):
    c = frozen_case(cid)
    enc = frozen_module(cid).encoder
    wav = _waves(c.lens, 33 + len(cid))
    L = wav.shape[1]
    T = enc.frame_geometry(L)[1]
    pack = enc.packed_geometry(c.lens, L, need_rows=[min(round(l / 320), T) for l in c.lens])
    return enc, wav, pack, enc.valid_frames(c.lens, L, T)


def frozen_reference(cid, layout, model=False, **mut):
    """-> hidden[b][i] fp64 [valid_b, d]"""
    c = frozen_case(cid)
    enc, wav, pack, _ = frozen_setup(cid)
    return R.frozen_encoder_train(enc, wav, list(c.lens), frozen_seed(), enc.dropout_rates(), pack if layout == "packed" else None, model, **mut)


@functools.lru_cache(maxsize=None)
def frozen_reference_cached(cid, layout):
    return frozen_reference(cid, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", FRONT_LAYOUTS)
@pytest.mark.parametrize("cid", [c.id for c in FROZEN_CASES])
def test_frozen_encoder_train_mode_hidden_states_against_fp64_with_the_host_masks(cid, layout, monkeypatch):
    monkeypatch.setenv("SC_FROZEN_DROPOUT", "1")
    monkeypatch.setenv("SC_VARLEN_PACK", "1" if layout == "packed" else "0")
    c = frozen_case(cid)
    _, wav, _, valid = frozen_setup(cid)
    ref = frozen_reference_cached(cid, layout)
    mod = frozen_module(cid).cuda().train()
    assert mod._pack_plan(wav.cuda(), list(c.lens)) is not None or layout == "padded", "this config must run on packed rows"
    with torch.no_grad():
        torch.manual_seed(FROZEN_TORCH_SEED)
        hs, _ = mod(wav.cuda(), torch.tensor(c.lens))
        hs = [h.float().cpu() for h in hs]
    assert len(hs) == mod.encoder.cfg.encoder_layers + 1
    for i, h in enumerate(hs):
        judge_rows(f"{cid}-{layout}/h{i}", torch.cat([h[b, :v] for b, v in enumerate(valid)]), torch.cat([ref[b][i] for b in range(len(valid))]))


@pytest.mark.gpu
@pytest.mark.parametrize("rate", ["dropout", "attention_dropout", "activation_dropout", "dropout_input"])
def test_pre_ln_encoder_still_refuses_train_mode_dropout(rate):
    from oracle.hubert_ref import HubertRefConfig
    from speechclip_amd.module.hubert import HubertConfig, HubertModel
    rates = dict(dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, dropout_input=0.0)
    rates[rate] = 0.1
    cfg = HubertConfig(**dataclasses.asdict(HubertRefConfig.tiny(layer_norm_first=True, extractor_mode="layer_norm", conv_bias=True)), **rates)
    torch.manual_seed(1)
    enc = HubertModel(cfg).cuda()
    wav = _waves((3000, 2000), 3).cuda()
    with pytest.raises(NotImplementedError):
        enc.extract_all_layers(wav, [3000, 2000], dropout_seed=7)
    hidden = enc.extract_all_layers(wav, [3000, 2000])[0]          # and without a seed it runs
    assert bool(torch.isfinite(hidden.float()).all())
