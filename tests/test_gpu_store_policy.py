"""Output-store policy (plain against write-through sc1 stores of the streaming kernels' 16-byte outputs): the decoder's
kernel-mask bits 4 / 8 (levels 0 / 1, mt_decoder_set_kernels), mt_vocoder_set_store_policy (one bit per stage) and
mt_encoder_set_store_policy. The policy changes where a written line waits (the XCD's L2 until the launch boundary, or
sent on at once), never a value, an address or the order of arithmetic, and visibility still comes from the kernel
boundary: policy-on must EQUAL policy-off bit for bit, eagerly, on graph capture and on replays with changed inputs (a
consumer that read a stale line would show there). No tolerance anywhere."""
import pytest
import torch

from conftest import make_decoder, make_generator, make_matcha

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
STEPS = 3
WT_BITS = 4 | 8  # DECK_WT0 | DECK_WT1


def _load(mod, seed):
    from matcha_hip import synthetic
    sd = {k: torch.from_numpy(v) for k, v in synthetic.make_state_dict(
        [(k, tuple(v.shape)) for k, v in mod.state_dict().items()], seed).items()}
    mod.load_state_dict(sd)
    return mod.to(DEV).eval()


@pytest.fixture(scope="module")
def dec160():
    return _load(make_decoder(160, "bf16"), 29)


def _dec_inputs(T, lens, seed):
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    mask = (torch.arange(T)[None] < torch.tensor(lens)[:, None]).float()[:, None]
    mu = (torch.randn(B, 80, T, generator=g) * mask).to(DEV)
    z = (torch.randn(B, 80, T, generator=g) * 0.667).to(DEV)
    return z, mu, mask.to(DEV)


def _solve(dec, kmask, graphs, inp, mv):
    from matcha_hip import runtime as rt
    z, mu, mask = inp
    eng = dec.engine()
    prev = rt.set_decoder_kernels(kmask)
    eng.set_graphs(graphs)
    try:
        out = eng.solve(dec.packed(DEV), z, 1.0, mu, mask, None, STEPS, solver="euler", max_valid=mv)
        torch.cuda.synchronize()
        return out.cpu()
    finally:
        rt.set_decoder_kernels(prev)
        eng.set_graphs(1)


# T = 200: 200 > T - 2 leaves level 1 on the general attention path; T = 204: both levels uniform
@pytest.mark.parametrize("T", [200, 204])
def test_decoder_solve_bit_identical(dec160, T):
    """Euler, 3 steps, the fused FeedForward on every level; eager, graph capture, then two replays with z and mu
    changed in between; both levels' bits together and each alone"""
    from matcha_hip import runtime as rt
    lens = [200, 137, 61]
    a, b = _dec_inputs(T, lens, 5), _dec_inputs(T, lens, 6)
    prev = rt.set_ffn_min_frames(0)
    try:
        base_a, base_b = _solve(dec160, 3, 0, a, 200), _solve(dec160, 3, 0, b, 200)
        assert torch.isfinite(base_a).all() and torch.isfinite(base_b).all()
        assert not torch.equal(base_a, base_b)
        for graphs, inp, base in ((0, a, base_a), (0, b, base_b), (1, a, base_a), (1, b, base_b), (1, a, base_a)):
            got = _solve(dec160, 3 | WT_BITS, graphs, inp, 200)
            assert torch.equal(got, base), (T, graphs, (got - base).abs().max())
        for bit in (4, 8):
            for inp, base in ((a, base_a), (b, base_b)):
                assert torch.equal(_solve(dec160, 3 | bit, 1, inp, 200), base), (T, bit)
    finally:
        rt.set_ffn_min_frames(prev)


def test_decoder_solve_bit_identical_unfused_ffn(dec160):
    """... with the FeedForward as two mt_vconv launches and x += o_b as its own launch (attn_uni_apply_kernel)"""
    from matcha_hip import runtime as rt
    a = _dec_inputs(204, [200, 137, 61], 7)
    prev = rt.set_ffn_min_frames(1 << 30)
    try:
        base = _solve(dec160, 3, 0, a, 200)
        for graphs in (0, 1, 1):
            assert torch.equal(_solve(dec160, 3 | WT_BITS, graphs, a, 200), base), graphs
    finally:
        rt.set_ffn_min_frames(prev)


@pytest.fixture(scope="module")
def gen():
    g = _load(make_generator("bf16"), 8)
    g.remove_weight_norm()
    return g


def test_vocoder_bit_identical(gen):
    """ragged batch (70 / 41 / 9 frames), the same three at full length, and the one-utterance calls: every stage's
    bit alone and all together"""
    T = 70
    lens = torch.tensor([70, 41, 9])
    mel = (torch.randn(3, 80, T, generator=torch.Generator().manual_seed(9)) * 2.1 - 5.5).to(DEV)
    eng = gen.engine()

    def run(mask):
        eng.set_store_policy(mask)
        try:
            with torch.inference_mode():
                rag = gen(mel, lengths=lens.to(DEV))
                full = gen(mel)
                one = [gen(mel[b:b + 1, :, :int(lens[b])].contiguous()) for b in range(3)]
            torch.cuda.synchronize()
        finally:
            eng.set_store_policy(0)
        return rag.cpu(), full.cpu(), [o.cpu() for o in one]

    rag0, full0, one0 = run(0)
    assert torch.isfinite(rag0).all() and torch.isfinite(full0).all()
    hop = rag0.shape[-1] // T
    for b in range(3):  # the ragged rows are the one-utterance calls, zero past their length
        n = hop * int(lens[b])
        assert torch.equal(rag0[b:b + 1, :, :n], one0[b]) and not rag0[b, :, n:].any()
    for mask in (1, 2, 4, 8, 15):
        rag, full, one = run(mask)
        assert torch.equal(rag, rag0), mask
        assert torch.equal(full, full0), mask
        for b in range(3):
            n = hop * int(lens[b])
            assert torch.equal(one[b], one0[b]) and torch.equal(rag[b:b + 1, :, :n], one[b]), (mask, b)


@pytest.mark.parametrize("mode", [0, 4])
def test_vocoder_bit_identical_pair_modes(gen, mode):
    """... with every pair as two per-layer launches (mt_rbconv / mt_vconv, set_pair(0)) and with every 128-channel
    pair fused (set_pair(4))"""
    lens = torch.tensor([70, 41, 9]).to(DEV)
    mel = (torch.randn(3, 80, 70, generator=torch.Generator().manual_seed(10)) * 2.1 - 5.5).to(DEV)
    eng = gen.engine()
    eng.set_pair(mode)
    try:
        outs = []
        for mask in (0, 15):
            eng.set_store_policy(mask)
            with torch.inference_mode():
                outs.append((gen(mel, lengths=lens).cpu(), gen(mel).cpu()))
        assert torch.isfinite(outs[0][0]).all()
        assert torch.equal(outs[1][0], outs[0][0]) and torch.equal(outs[1][1], outs[0][1])
    finally:
        eng.set_store_policy(0)
        eng.set_pair(1)


@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
def test_encoder_bit_identical(precision):
    m = _load(make_matcha(1, "fp32"), 1)
    m.set_precision("fp32", encoder_precision=precision)
    g = torch.Generator().manual_seed(3)
    xl = torch.tensor([50, 33, 7])
    x = torch.randint(0, 178, (3, 50), generator=g)
    x = (x * (torch.arange(50)[None] < xl[:, None])).to(DEV)
    xl = xl.to(DEV)
    eng = m.encoder.engine()
    outs = []
    try:
        for mode in (0, 1, 0):
            eng.set_store_policy(mode)
            with torch.inference_mode():
                mu, logw, _ = m.encoder(x, xl)
            torch.cuda.synchronize()
            outs.append((mu.cpu(), logw.cpu()))
    finally:
        eng.set_store_policy(0)
    assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][1]).all()
    for mu, logw in outs[1:]:
        assert torch.equal(logw, outs[0][1])
        assert torch.equal(mu, outs[0][0])


def test_bench_step_bit_identical():
    """B = 4, 3 ODE steps through MatchaTTS.synthesize + Generator + Denoiser: every policy on against every policy off"""
    import bench
    from matcha_hip import runtime as rt
    m, g, den, _, _ = bench.build_models(DEV, "bf16", 1234)
    x, xl = bench.shard_inputs(0, 1, 4, 4327)
    x, xl = x.to(DEV), xl.to(DEV)

    def step(on):
        prev = rt.set_decoder_kernels(3 | (WT_BITS if on else 0))
        g.engine().set_store_policy(15 if on else 0)
        m.encoder.engine().set_store_policy(1 if on else 0)
        try:
            torch.manual_seed(7)  # the same CFM noise z for every run (synthesize draws it with torch.randn_like)
            with torch.inference_mode():
                mel, yl, wav = bench.step(m, g, den, x, xl, 3, True)
            torch.cuda.synchronize()
        finally:
            rt.set_decoder_kernels(prev)
            g.engine().set_store_policy(0)
            m.encoder.engine().set_store_policy(0)
        return mel.cpu(), yl.cpu(), wav.cpu()

    base = step(False)
    assert torch.isfinite(base[0]).all() and torch.isfinite(base[2]).all()
    for _ in range(2):  # graph capture, then replay
        got = step(True)
        assert torch.equal(got[1], base[1])
        assert torch.equal(got[0], base[0]), (got[0] - base[0]).abs().max()
        assert torch.equal(got[2], base[2])


def test_setters_refuse_unknown_modes(gen):
    """an unknown mode is an error from the setter itself: no launch, no HIP call, the setting unchanged"""
    from matcha_hip import runtime as rt
    eng = gen.engine()  # the v1 generator: 4 stages
    for bad in (16, 31, -1, 1 << 20):
        with pytest.raises(RuntimeError, match="store_policy"):
            eng.set_store_policy(bad)
    eng.set_store_policy(15)
    eng.set_store_policy(0)
    enc = make_matcha(1, "fp32").encoder.engine()
    for bad in (2, 16, -1):
        with pytest.raises(RuntimeError, match="store_policy"):
            enc.set_store_policy(bad)
    enc.set_store_policy(1)
    enc.set_store_policy(0)
    # the decoder's bits ride on its kernel mask, which keeps its documented bits and drops the rest
    prev = rt.set_decoder_kernels(3 | WT_BITS | 16 | 1024)
    try:
        assert rt.set_decoder_kernels(prev) == 3 | WT_BITS
    finally:
        rt.set_decoder_kernels(prev)
