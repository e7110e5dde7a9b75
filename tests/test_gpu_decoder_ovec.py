"""Decoder kernel-variant bit 1 (DECK_OVEC, mt_decoder_set_kernels): the query-independent attention's vector o_b is
computed in the first estimator evaluation of a solve only and kept per transformer block for the later ones, instead
of attn_uni_part_kernel + attn_uni_vec_kernel in every evaluation. o_b is a function of the weights and of the number
of masked frames only (the masked frames of a transformer chain's input hold res_conv.bias in every evaluation:
model.py:773-790, 697; DESIGN "o_b once per solve"), so mask 3 must EQUAL mask 1 bit for bit: eagerly, on graph
capture and on replays (a slot left by the previous solve must never be read), for both solvers, with a second block
per chain, with speaker conditioning, and through the bench's text->wav step. No tolerance anywhere."""
import pytest
import torch

from conftest import DEC, make_decoder

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
T = 48
STEPS = 3


def _load(dec, seed):
    from matcha_hip import synthetic
    sd = {k: torch.from_numpy(v) for k, v in synthetic.make_state_dict(
        [(k, tuple(v.shape)) for k, v in dec.state_dict().items()], seed).items()}
    dec.load_state_dict(sd)
    return dec.to(DEV).eval()


@pytest.fixture(scope="module")
def dec160():
    return _load(make_decoder(160, "bf16"), 29)


@pytest.fixture(scope="module")
def dec2blocks():
    import model
    return _load(model.Decoder(in_channels=160, out_channels=80, precision="bf16", **{**DEC, "n_blocks": 2}), 31)


@pytest.fixture(scope="module")
def dec224():
    return _load(make_decoder(224, "bf16"), 37)


def _inputs(lens, seed, hole=None, spk=0):
    """(z, mu, mask, spks) on the device; hole = (utterance, first, last + 1): those frames' mask set to zero"""
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    mask = (torch.arange(T)[None] < torch.tensor(lens)[:, None]).float()[:, None]
    if hole is not None:
        mask[hole[0], 0, hole[1]:hole[2]] = 0.
    mu = (torch.randn(B, 80, T, generator=g) * mask).to(DEV)
    z = (torch.randn(B, 80, T, generator=g) * 0.667).to(DEV)
    spks = torch.randn(B, spk, generator=g).to(DEV) if spk else None
    return z, mu, mask.to(DEV), spks


def _solve(dec, kmask, graphs, inp, solver, mv):
    from matcha_hip import runtime as rt
    z, mu, mask, spks = inp
    eng = dec.engine()
    prev = rt.set_decoder_kernels(kmask)
    eng.set_graphs(graphs)
    try:
        out = eng.solve(dec.packed(DEV), z, 1.0, mu, mask, spks, STEPS, solver=solver, max_valid=mv)
        torch.cuda.synchronize()
        return out.cpu()
    finally:
        rt.set_decoder_kernels(prev)
        eng.set_graphs(1)


# (lens, max_valid, hole): the uniform path at both levels; at level 0 only (level 1 general: 47 > T - 2); general
# attention at both (max_valid unknown: the bit must be a no-op); a mask with a hole on the uniform path
SHAPES = [
    ([46, 31, 5], 46, None),
    ([47, 31, 5], 47, None),
    ([46, 31, 5], 0, None),
    ([46, 31, 5], 46, (1, 10, 14)),
]


def _check_shapes(dec, solver, spk=0):
    for lens, mv, hole in SHAPES:
        a = _inputs(lens, 5, hole, spk)
        # the same geometry (the same graph, the same workspace) with other z / mu and two utterances' lengths swapped:
        # every o_b changes (it depends on the utterance's masked-frame count), so a stale slot would show
        b = _inputs([lens[1], lens[0], lens[2]], 6, (0,) + hole[1:] if hole else None, spk)
        base_a, base_b = _solve(dec, 1, 0, a, solver, mv), _solve(dec, 1, 0, b, solver, mv)
        assert torch.isfinite(base_a).all() and torch.isfinite(base_b).all()
        assert not torch.equal(base_a, base_b)
        # eager, then graph capture, then replays alternating the inputs
        for graphs, inp, base in ((0, a, base_a), (0, b, base_b), (1, a, base_a), (1, a, base_a), (1, b, base_b),
                                  (1, a, base_a), (1, b, base_b)):
            got = _solve(dec, 3, graphs, inp, solver, mv)
            assert torch.equal(got, base), (lens, mv, hole, graphs, (got - base).abs().max())
        # bit 1 alone (the generic final projection) on the same graph geometry
        assert torch.equal(_solve(dec, 2, 1, a, solver, mv), base_a), (lens, mv, hole)


@pytest.mark.parametrize("solver", ["euler", "midpoint"])
def test_ovec_bit_identical_solve(dec160, solver):
    _check_shapes(dec160, solver)


@pytest.mark.parametrize("solver", ["euler", "midpoint"])
def test_ovec_bit_identical_solve_fused_ffn(dec160, solver):
    """... with the fused FeedForward on every level: it adds o_b itself, straight from the block's slot"""
    from matcha_hip import runtime as rt
    prev = rt.set_ffn_min_frames(0)
    try:
        _check_shapes(dec160, solver)
    finally:
        rt.set_ffn_min_frames(prev)


@pytest.mark.parametrize("mode", [0, 2])
def test_ovec_bit_identical_conv_paths(dec160, mode):
    """... on the decoder's other conv paths (set_vconv: 0 the generic conv kernel, which masks its inputs in the
    prologue instead of reading stored-masked tensors; 2 GroupNorm as its own pass): the masked rows are constant there
    for the same reason"""
    eng = dec160.engine()
    eng.set_vconv(mode)
    try:
        _check_shapes(dec160, "midpoint")
    finally:
        eng.set_vconv(1)


@pytest.mark.parametrize("solver", ["euler", "midpoint"])
def test_ovec_bit_identical_two_blocks(dec2blocks, solver):
    """a chain's second block: its input at the masked frames is the first block's output on the constant row"""
    _check_shapes(dec2blocks, solver)


@pytest.mark.parametrize("solver", ["euler", "midpoint"])
def test_ovec_bit_identical_speaker(dec224, solver):
    _check_shapes(dec224, solver, spk=64)


def _counts(log):
    from matcha_hip import runtime as rt
    c = {"part": 0, "vec": 0, "apply": 0, "ffn": 0}
    for r in log:
        ef = r["ef"]
        if ef == rt.UNI_LOG_PART:
            c["part"] += 1
        elif ef == rt.UNI_LOG_VEC:
            c["vec"] += 1
        elif ef == rt.UNI_LOG_APPLY:
            c["apply"] += 1
        elif ef == rt.FFN_LOG or (ef < 0x10000 and ef & 64 and r["M"] == 1024):  # fused, or FF1 (VE_SNAKE) on mt_vconv
            c["ffn"] += 1
    return c


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("solver", ["euler", "midpoint"])
def test_ovec_launch_counts(dec160, solver, fused):
    """N blocks on the uniform path, S evaluations: mask 1 launches part and vec N * S times, mask 3 N times; x += o_b
    (its own launch, or inside the fused FeedForward) and the FeedForward stay at one per block and evaluation"""
    from matcha_hip import runtime as rt
    S = STEPS if solver == "euler" else 2 * STEPS
    nb = 6  # transformer blocks of the n_blocks = 1 U-Net: 2 at level 0, 4 at level 1
    prev = rt.set_ffn_min_frames(0) if fused else None
    sel = rt.vconv_log_select(rt.LOG_CONV)

    def counts(kmask, inp, mv):
        rt.vconv_log_start(20000)  # an armed log takes the solve off its graph: eager launches
        try:
            _solve(dec160, kmask, 1, inp, solver, mv)
        finally:
            log = rt.vconv_log_stop(20000)
        return _counts(log)

    try:
        # by default the log holds conv launches only (its other readers expect conv variants) ...
        c = counts(3, _inputs(SHAPES[0][0], 5), SHAPES[0][1])
        assert c == {"part": 0, "vec": 0, "apply": 0, "ffn": 0 if fused else nb * S}, c
        rt.vconv_log_select(rt.LOG_CONV | rt.LOG_AUX)  # ... and these launches on request
        for (lens, mv, hole), N in zip(SHAPES, (6, 2, 0, 6)):
            inp = _inputs(lens, 5, hole)
            got = {kmask: counts(kmask, inp, mv) for kmask in (1, 3)}
            napply = 0 if fused else N * S
            assert got[1] == {"part": N * S, "vec": N * S, "apply": napply, "ffn": nb * S}, (lens, mv, got[1])
            assert got[3] == {"part": N, "vec": N, "apply": napply, "ffn": nb * S}, (lens, mv, got[3])
    finally:
        rt.vconv_log_select(sel)
        if fused:
            rt.set_ffn_min_frames(prev)


def test_ovec_bit_identical_bench_step():
    import bench
    from matcha_hip import runtime as rt
    m, g, den, _, _ = bench.build_models(DEV, "bf16", 1234)
    x, xl = bench.shard_inputs(0, 1, 6, 4327)
    x, xl = x.to(DEV), xl.to(DEV)

    def step(kmask):
        prev = rt.set_decoder_kernels(kmask)
        try:
            torch.manual_seed(7)  # the same CFM noise z for every run (synthesize draws it with torch.randn_like)
            with torch.inference_mode():
                mel, yl, wav = bench.step(m, g, den, x, xl, 10, True)
            torch.cuda.synchronize()
        finally:
            rt.set_decoder_kernels(prev)
        return mel.cpu(), yl.cpu(), wav.cpu()

    base = step(1)
    assert torch.isfinite(base[0]).all() and torch.isfinite(base[2]).all()
    for _ in range(2):  # graph capture, then replay
        got = step(3)
        assert torch.equal(got[1], base[1])
        assert torch.equal(got[0], base[0]), (got[0] - base[0]).abs().max()
        assert torch.equal(got[2], base[2])
