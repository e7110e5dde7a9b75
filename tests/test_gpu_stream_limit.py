"""Streamed level control on the GPU (csrc/mt_limiter.hip's range kernels, hifigan/output.py's gain_db=,
hifigan/stream.py). Every comparison is bit for bit: mt_peak_envelope_range and mt_limit_range against
the whole-row kernels, with everything outside what they may read poisoned; the one-shot fixed-gain stage against
limiter.limit_fixed_ref and the encoder references; the concatenated chunks of a stream against the one-shot call of
the same stage.
"""
import numpy as np
import pytest
import torch

from conftest import make_generator

from matcha_hip import audio_out as ao
from matcha_hip import limiter as lm

pytestmark = pytest.mark.gpu
DEV = "cuda"
CEIL_DB = -1.0
C = 10.0 ** (CEIL_DB / 20.0)
C32 = np.float32(C)
POISON = 1e30  # finite: a NaN counts as absent in the envelope and would hide a read
SENTINEL = -7.0


def _noise(n, seed, scale=0.1):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)


def _batch(rows, L=None, fill=0.0):
    L = max(max(len(r) for r in rows), 1) if L is None else L
    x = np.full((len(rows), L), fill, np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    return torch.from_numpy(x).to(DEV), torch.tensor([len(r) for r in rows], dtype=torch.int32, device=DEV)


# ---- mt_peak_envelope_range ----------------------------------------------------------------------------------------

ENV_N = 1029  # two tiles of 512 and five samples
ENV_RANGES = [(0, 1), (0, ENV_N), (511, 3), (ENV_N - 1, 1), (1000, 100), (ENV_N, 5), (ENV_N + 300, 7), (3, 1024)]


def test_envelope_range_is_the_whole_row_kernels_bits():
    from matcha_hip import runtime as rt
    assert rt.ENVELOPE_TILE == 512
    plan4 = rt.resample_plan(16000, 64000)
    reach = lm.envelope_reach(plan4.half)
    assert reach == 10
    rows = [_noise(ENV_N, 1, 0.3), _noise(513, 2, 0.3), np.zeros(0, np.float32), _noise(700, 3, 0.3)]
    L = ENV_N + 71
    x, lens = _batch(rows, L)
    full = rt.peak_envelope(x, lens, plan4)
    for b, r in enumerate(rows):
        assert np.array_equal(full[b, :len(r)].cpu().numpy(), lm.envelope_ref(r)), b
    for i_lo, cnt in ENV_RANGES:
        a = x.clone()
        a[:, i_lo + cnt + reach:] = POISON  # past the documented last read, i_lo + cnt - 1 + (half + 3) / 4
        env = torch.full((len(rows), L), SENTINEL, device=DEV)
        got = rt.peak_envelope_range(a, lens, plan4, i_lo, cnt, env)
        assert got is env
        want = torch.full_like(env, SENTINEL)
        for b, r in enumerate(rows):
            lo, hi = min(i_lo, len(r)), min(i_lo + cnt, len(r))
            want[b, lo:hi] = full[b, lo:hi]
        assert torch.equal(env, want), (i_lo, cnt, (env != want).nonzero()[:4].tolist())
    with pytest.raises(Exception, match="peak_envelope_range"):
        rt.peak_envelope_range(x, lens, plan4, 0, 0, full.clone())
    with pytest.raises(Exception, match="peak_envelope_range"):
        rt.peak_envelope_range(x, lens, plan4, -1, 4, full.clone())
    with pytest.raises(ValueError, match="env"):
        rt.peak_envelope_range(x, lens, plan4, 0, 4, full[:, :-1].contiguous())


# ---- mt_limit_range --------------------------------------------------------------------------------------------------

LIM_N = 5000  # two tiles of 2048 and 904 samples


def _limit_case(W):
    """rows, their envelopes (over the ceiling at a good part of the samples), gains and mt_limit's result"""
    from matcha_hip import runtime as rt
    xs = [_noise(LIM_N, 10, 0.3), _noise(2100, 11, 0.3), np.zeros(0, np.float32)]
    es = [np.abs(_noise(LIM_N, 12, 0.5)), np.abs(_noise(2100, 13, 0.4)), np.zeros(0, np.float32)]
    L = LIM_N + 37
    x, lens = _batch(xs, L)
    e, _ = _batch(es, L)
    gain = torch.tensor([1.7, 0.9, 3.0], dtype=torch.float32, device=DEV)
    ones = torch.ones(3, dtype=torch.float32, device=DEV)
    y, g_out, red = rt.limit(x, e, lens, (ones, ones.double()), 1.0, C, W, gain_in=gain)
    assert torch.equal(g_out, gain)  # level 1 at mean square 1 leaves the gain as it stands
    for b in range(2):
        s = lm.gain_curve_ref(es[b], gain[b].item(), C32, W)
        assert np.array_equal(y[b, :len(xs[b])].cpu().numpy(), lm.apply_ref(xs[b], np.float32(gain[b].item()), s))
        assert float(red[b]) == s.min() < 1.0
    return xs, es, x, e, lens, gain, y, red


@pytest.mark.parametrize("W", (1, 2, 80, 2048))
def test_limit_range_is_the_whole_row_kernels_bits(W):
    from matcha_hip import runtime as rt
    T = rt.LIMIT_TILE
    assert T == 2048
    xs, es, x, e, lens, gain, y, _ = _limit_case(W)
    n = LIM_N
    ranges = [(0, 100), (0, 1), (T - 48, 100), (T - 1, 2), (n - 1000, 1000), (100, max(W - 1, 1)), (n - 10, 50),
              (n, 10), (n + 1000, 10), (0, n), (1, 2 * T + 5), (2099, 3)]
    for i_lo, cnt in ranges:
        xa = torch.full_like(x, POISON)
        xa[:, i_lo:i_lo + cnt] = x[:, i_lo:i_lo + cnt]  # of audio, the range alone
        ea = torch.full_like(e, POISON)
        lo, hi = max(i_lo - (W - 1), 0), i_lo + cnt + W - 1
        ea[:, lo:hi] = e[:, lo:hi]                      # of env, [i_lo - (W - 1), i_lo + cnt + W - 2]
        red = torch.ones(3, dtype=torch.float32, device=DEV)
        out, out_cnt = rt.limit_range(xa, ea, lens, gain, C, W, i_lo, cnt, red)
        assert out.shape == (3, cnt) and out.dtype == torch.float32
        want_cnt = [min(max(len(r) - i_lo, 0), cnt) for r in xs]
        assert out_cnt.tolist() == want_cnt, (W, i_lo, cnt)
        for b, k in enumerate(want_cnt):
            assert torch.equal(out[b, :k], y[b, i_lo:i_lo + k]), (W, i_lo, cnt, b)
            assert not out[b, k:].any(), (W, i_lo, cnt, b)  # zero past the row's end
            s = lm.gain_curve_ref(es[b], gain[b].item(), C32, W)[i_lo:i_lo + k]
            assert float(red[b]) == (s.min() if k else 1.0), (W, i_lo, cnt, b)
    red = torch.ones(3, dtype=torch.float32, device=DEV)
    for kw, match in ((dict(i_lo=0, cnt=0), "limit_range"), (dict(i_lo=-1, cnt=3), "limit_range"),
                      (dict(i_lo=0, cnt=3, W=2049), "window")):
        args = dict(W=W)
        args.update(kw)
        with pytest.raises(Exception, match=match):
            rt.limit_range(x, e, lens, gain, C, args["W"], args["i_lo"], args["cnt"], red)
    with pytest.raises(ValueError, match="gain"):
        rt.limit_range(x, e, lens, gain.double(), C, W, 0, 4, red)
    with pytest.raises(ValueError, match="reduction"):
        rt.limit_range(x, e, lens, gain, C, W, 0, 4, red[:2])


@pytest.mark.parametrize("W", (1, 80, 2048))
def test_running_reduction_over_consecutive_ranges(W):
    from matcha_hip import runtime as rt
    xs, es, x, e, lens, gain, y, red_full = _limit_case(W)
    cuts = [0, 1, 2047, 2049, 2100, 4500, LIM_N + 50]
    red = torch.ones(3, dtype=torch.float32, device=DEV)
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        out, _ = rt.limit_range(x, e, lens, gain, C, W, lo, hi - lo, red)
        parts.append(out)
        for b in range(2):
            s = lm.gain_curve_ref(es[b], gain[b].item(), C32, W)[:hi]
            assert float(red[b]) == s.min(), (W, hi, b)
    assert torch.equal(red, red_full) and float(red[2]) == 1.0
    assert torch.equal(torch.cat(parts, dim=1)[:, :y.shape[1]], y)


def test_range_rows_do_not_depend_on_the_batch():
    from matcha_hip import runtime as rt
    plan4 = rt.resample_plan(22050, 88200)
    W, i_lo, cnt = 110, 1000, 3500
    lens = [2 * rt.LIMIT_TILE + 777, 1, 0, 1700, 3001]
    base = [_noise(n, 60 + i, 0.4) for i, n in enumerate(lens)]
    gains = [2.0, 1.0, 5.0, 0.5, 3.0]

    def run(x, ll, g):
        env = torch.full_like(x, SENTINEL)
        rt.peak_envelope_range(x, ll, plan4, 0, x.shape[1], env)  # everything the limiter's range reads
        red = torch.ones(x.shape[0], dtype=torch.float32, device=DEV)
        out, out_cnt = rt.limit_range(x, env, ll, torch.tensor(g, dtype=torch.float32, device=DEV), C, W, i_lo, cnt,
                                      red)
        return env, out, out_cnt, red

    singles = [run(*_batch([r], fill=7.0), [g]) for r, g in zip(base, gains)]
    assert float(singles[0][3][0]) < 1.0
    for L, perm in ((max(lens), [0, 1, 2, 3, 4]), (max(lens) + 1234, [3, 2, 4, 0, 1])):
        env, out, out_cnt, red = run(*_batch([base[b] for b in perm], L=L, fill=7.0), [gains[b] for b in perm])
        for row, b in enumerate(perm):
            e1, o1, c1, r1 = singles[b]
            n = lens[b]
            assert torch.equal(env[row, :n], e1[0, :n]) and (env[row, n:] == SENTINEL).all(), (L, b)
            assert torch.equal(out[row], o1[0]) and out_cnt[row] == c1[0] and red[row] == r1[0], (L, b)


# ---- the one-shot fixed-gain stage -----------------------------------------------------------------------------------

def burst_signal(fs, seed=0, seconds=1.0):
    """noise of sigma 0.02 with twelve 8-sample bursts of sigma 0.5 (DESIGN §23's signal)"""
    rng = np.random.default_rng(seed)
    n = int(seconds * fs)
    x = rng.standard_normal(n) * 0.02
    for p in rng.choice(np.arange(200, n - 200, 400), 12, replace=False):
        x[p:p + 8] = rng.standard_normal(8) * 0.5
    return x.astype(np.float32)


def _encoded(y):
    q = ao.pcm16_ref(y, np.float32(1.0))
    return {"f32": ao.f32_ref(y, np.float32(1.0)), "pcm16": q, "mulaw": ao.mulaw_ref(q)}


@pytest.mark.parametrize("fs", (8000, 22050))
def test_one_shot_fixed_gain_equals_the_specification(fs):
    from hifigan.output import AudioOutput, Limited
    W = lm.window_samples(fs, 5.0)
    rows = [burst_signal(fs, 1), burst_signal(fs, 2)[:fs // 2 + 13], np.zeros(0, np.float32)]
    dbs = [6.0, 20.0, 3.0]
    x, ll = _batch(rows, fill=9.0)
    for override in (None, dbs):
        use = [6.0] * 3 if override is None else dbs
        spec = [lm.limit_fixed_ref(r, db, CEIL_DB, W) for r, db in zip(rows, use)]
        plain = [(lm.fixed_gain_ref(db) * r).astype(np.float32) for r, db in zip(rows, use)]
        assert spec[0][1] < 1.0 and spec[1][1] < 1.0 and not np.array_equal(spec[0][0], plain[0])
        g = [float(lm.fixed_gain_ref(db)) for db in use]
        for enc in ao.ENCODINGS:
            lim = AudioOutput(fs, source_rate=fs, gain_db=6.0, true_peak=CEIL_DB, limiter=5.0, encoding=enc,
                              limiter_passes=5)  # ignored with gain_db
            fix = AudioOutput(fs, source_rate=fs, gain_db=6.0, encoding=enc)
            for stage, ys in ((lim, [s[0] for s in spec]), (fix, plain)):
                out = stage.finish(x, ll, gain_db=override)
                assert out.sample_rate == fs and torch.equal(out.lengths, ll) and out.gain.tolist() == g
                for b, yr in enumerate(ys):
                    assert np.array_equal(out.audio[b, :len(yr)].cpu().numpy(), _encoded(yr)[enc]), (fs, enc, b)
                # __call__ (lengths None: every row is L samples long, as row 0 is)
                assert torch.equal(stage(x[:, None], None, gain_db=override).audio[0], out.audio[0])
        rep = lim.limited(x, ll, gain_db=override)
        assert isinstance(rep, Limited) and rep.gain.tolist() == g and rep.trim.tolist() == [1.0] * 3
        assert rep.reduction.tolist() == [float(s[1]) for s in spec]
        for b, s in enumerate(spec):
            assert np.array_equal(rep.audio[b, :len(rows[b])].cpu().numpy(), s[0]), b
    with pytest.raises(ValueError, match="device tensor"):
        lim.finish(x, ll, gain_db=torch.tensor(dbs, device=DEV))
    with pytest.raises(ValueError, match="entries"):
        lim.finish(x, ll, gain_db=[1.0, 2.0])


# ---- the stream --------------------------------------------------------------------------------------------------------

B, T = 6, 64
LENGTHS = [61, 32, 17, 1, 0, 45]
STRENGTH = 0.00025


@pytest.fixture(scope="module")
def ctx():
    """test_gpu_stream.py's generator, denoiser, mel and lengths, and the one-shot denoised audio"""
    from hifigan.denoiser import Denoiser
    from matcha_hip import synthetic
    g = make_generator("bf16")
    sd = synthetic.make_state_dict([(k, tuple(v.shape)) for k, v in g.state_dict().items()], 8)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    g = g.to(DEV).eval()
    g.remove_weight_norm()
    den = Denoiser(g, mode="zeros")
    mel = (torch.randn(B, 80, T, generator=torch.Generator().manual_seed(9)) * 2.1 - 5.5).to(DEV)
    lens = torch.tensor(LENGTHS, device=DEV)
    clean = den(g(mel, lens).squeeze(1), STRENGTH, lens)
    torch.cuda.synchronize()
    return dict(g=g, den=den, mel=mel, lens=lens, clean=clean.clone(), ref={})


def _stitch(chunks, n_rows):
    """test_gpu_stream.py's: -> (the concatenated valid samples of each row, number of chunks); checks offset /
    lengths / done"""
    parts = [[] for _ in range(n_rows)]
    total = [0] * n_rows
    done = [0] * n_rows
    n = 0
    for ch in chunks:
        n += 1
        assert ch.audio.shape[0] == n_rows and ch.lengths.dtype == torch.int32 and ch.done.dtype == torch.bool
        ln, off, dn = ch.lengths.tolist(), ch.offset.tolist(), ch.done.tolist()
        for b in range(n_rows):
            assert 0 <= ln[b] <= ch.audio.shape[1]
            assert off[b] == total[b], (n, b, off[b], total[b])
            parts[b].append(ch.audio[b, :ln[b]].clone())
            total[b] += ln[b]
            done[b] += int(dn[b])
    assert done == [1] * n_rows, done
    return [torch.cat(p) for p in parts], n


def _one_shot(ctx, rate, enc, limiter):
    """per (rate, encoding, limiter): the stage, the per-row gains that put every row's true peak 12 dB over the
    ceiling, the one-shot result and report; computed once"""
    from hifigan.output import AudioOutput
    from matcha_hip import runtime as rt
    key = (rate, enc, limiter)
    if key not in ctx["ref"]:
        tp = AudioOutput(rate).measure(ctx["clean"], ctx["lens"]).true_peak_db.tolist()
        gdb = [CEIL_DB + 12.0 - v if np.isfinite(v) else 0.0 for v in tp]
        o = AudioOutput(rate, gain_db=0.0, true_peak=CEIL_DB, limiter=limiter, encoding=enc)
        ref = o(ctx["clean"], ctx["lens"], gain_db=gdb)
        red = None
        if limiter is not None:
            if rate != 22050:
                res, res_lens = rt.resample(ctx["clean"], rt.resample_plan(22050, rate), ctx["lens"], lmul=256)
            else:
                res, res_lens = ctx["clean"], (ctx["lens"] * 256).to(torch.int32)
            red = o.limited(res, res_lens, gain_db=gdb).reduction
        ctx["ref"][key] = (o, gdb, ref, red)
    return ctx["ref"][key]


@pytest.mark.parametrize("rate,enc,limiter,chunk,first", [
    (8000, "mulaw", 5.0, 16, 8), (16000, "pcm16", 5.0, 16, 8), (22050, "f32", 5.0, 16, 8),
    (8000, "pcm16", 256.0, 16, 8),   # W = 2048, larger than a chunk
    (16000, "pcm16", None, 16, 8),   # the fixed gain alone
    (16000, "pcm16", 5.0, 5, None), (22050, "f32", None, 5, None)])
def test_stream_equals_one_shot(ctx, rate, enc, limiter, chunk, first):
    from hifigan.stream import WaveStreamer
    o, gdb, ref, red = _one_shot(ctx, rate, enc, limiter)
    s = WaveStreamer(ctx["g"], ctx["den"], o, chunk_frames=chunk, first_chunk_frames=first, strength=STRENGTH)
    rows, n = _stitch(s(ctx["mel"], ctx["lens"], gain_db=gdb), B)
    assert n == len(s.schedule(LENGTHS)) and n > 1
    ref_lens = ref.lengths.tolist()
    for b, r in enumerate(rows):
        assert r.dtype == ref.audio.dtype and r.numel() == ref_lens[b], (b, r.numel(), ref_lens[b])
        assert torch.equal(r, ref.audio[b, :ref_lens[b]]), b
    _, _, unlimited, _ = _one_shot(ctx, rate, enc, None)
    if limiter is None:
        assert s.reduction is None
        return
    assert torch.equal(s.reduction, red)
    # the limiter worked: a stream in which it never did would pass the equalities above vacuously
    for b, nf in enumerate(LENGTHS):
        if nf >= 17:
            assert float(red[b]) < 1.0, (b, float(red[b]))
    assert float(red[4]) == 1.0  # the empty row
    n0 = ref_lens[0]
    assert not torch.equal(ref.audio[0, :n0], unlimited.audio[0, :n0])


def test_stage_gain_without_override_and_refusals(ctx):
    """gain_db= of the stage itself for every row; an override on a stage without gain_db= is refused"""
    from hifigan.output import AudioOutput
    from hifigan.stream import WaveStreamer
    tp0 = float(AudioOutput(16000).measure(ctx["clean"], ctx["lens"]).true_peak_db[0])
    o = AudioOutput(16000, gain_db=CEIL_DB + 12.0 - tp0, true_peak=CEIL_DB, limiter=5.0, encoding="pcm16")
    ref = o(ctx["clean"], ctx["lens"])
    s = WaveStreamer(ctx["g"], ctx["den"], o, chunk_frames=16, strength=STRENGTH)
    rows, _ = _stitch(s(ctx["mel"], ctx["lens"]), B)
    for b, r in enumerate(rows):
        assert torch.equal(r, ref.audio[b, :int(ref.lengths[b])]), b
    assert float(s.reduction[0]) < 1.0
    with pytest.raises(ValueError, match="device tensor"):
        s(ctx["mel"], ctx["lens"], gain_db=torch.zeros(B, device=DEV))
    with pytest.raises(ValueError, match="without gain_db"):
        WaveStreamer(ctx["g"], ctx["den"], AudioOutput(16000))(ctx["mel"], ctx["lens"], gain_db=[0.0] * B)
    for bad in (AudioOutput(16000, normalize="rms"), AudioOutput(16000, loudness=-16.0, limiter=5.0)):
        with pytest.raises(ValueError, match="whole utterance"):
            WaveStreamer(ctx["g"], ctx["den"], bad)
