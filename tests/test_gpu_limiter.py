"""Look-ahead true-peak limiter on the GPU (csrc/mt_limiter.hip): mt_peak_envelope, mt_limit and the
`limiter=` path of hifigan.output.AudioOutput against the CPU specification matcha_hip/limiter.py. Every comparison
is bit for bit; the one tolerance is the 1e-9 LU between the loudness meter on the GPU and on the CPU (the
K-weighting scan's own margin), on signals whose samples are first shown equal.

A stage result is compared with limiter_ref run from the CPU's own measurement E of the input: the GPU's E differs
from it by some 1e-13 relative, which moves the fp32 gain only when level / sqrt(E) lies that close to a rounding
boundary of fp32 (odds of a few in a million per gain).
"""
import math

import numpy as np
import pytest
import torch

from conftest import make_generator, make_matcha

from matcha_hip import audio_out as ao
from matcha_hip import join as jn
from matcha_hip import limiter as lm
from matcha_hip import loudness as ld

pytestmark = pytest.mark.gpu
DEV = "cuda"
RATES = (8000, 22050)
CEIL_DB = -1.0
C = 10.0 ** (CEIL_DB / 20.0)
C32 = np.float32(C)


def _noise(n, seed, scale=0.1):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)


def burst_signal(fs, seed=0, seconds=2.0):
    """noise of sigma 0.02 with twelve 8-sample bursts of sigma 0.5 (test_limiter_host.py's signal)"""
    rng = np.random.default_rng(seed)
    n = int(seconds * fs)
    x = rng.standard_normal(n) * 0.02
    for p in rng.choice(np.arange(200, n - 200, 400), 12, replace=False):
        x[p:p + 8] = rng.standard_normal(8) * 0.5
    return x.astype(np.float32)


def _batch(rows, L=None, fill=None):
    """rows: list of fp32 arrays -> (x [B, L] host, lens); the padding holds `fill` (a value, NaN included)"""
    L = max(max(len(r) for r in rows), 1) if L is None else L
    x = np.zeros((len(rows), L), dtype=np.float32) if fill is None else np.full((len(rows), L), fill, np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    return torch.from_numpy(x), [len(r) for r in rows]


def _np(t):
    return t.detach().cpu().numpy()


_REF = {}


def _limiter_ref(x, fs, target, ms=5.0, passes=3):
    """limiter_ref and what the stage delivers from it, computed once per case:
    (y, g, reduction, trim, delivered f32, its LUFS)"""
    key = (x.tobytes(), fs, target, ms, passes)
    if key not in _REF:
        y, g, red, trim = lm.limiter_ref(x, fs, target, CEIL_DB, lm.window_samples(fs, ms), passes)
        d = ao.f32_ref(y, trim)
        _REF[key] = (y, g, red, trim, d, ld.lufs(ld.loudness_ref(d, fs)[0]))
    return _REF[key]


@pytest.mark.parametrize("fs", RATES)
def test_envelope_matches_the_specification(fs):
    from matcha_hip import runtime as rt
    T = rt.ENVELOPE_TILE
    assert T == 512  # 4 T = the true-peak kernel's tile: 511, 512, 513 are T - 1, T, T + 1 of both
    plan4 = rt.resample_plan(fs, 4 * fs)
    rows = [_noise(n, 200 + i, 0.3) for i, n in enumerate((1, 2, T - 1, T, T + 1, 2 * T + 5))]
    # the largest inter-sample peak of a row left of, across and right of a tile boundary: two equal neighbours
    for k in (T - 2, T - 1, T, 2 * T - 1):
        r = _noise(2 * T + 5, 300 + k, 0.02)
        r[k] = r[k + 1] = 0.7
        p = lm.envelope_ref(r)
        assert p[k] == p[k + 1] == p.max() > np.float32(0.7)  # between the two, and counted against both
        rows.append(r)
    rows.append(np.zeros(0, np.float32))
    for fill in (np.nan, 50.0):
        x, ll = _batch(rows, L=2 * T + 77, fill=fill)
        env = _np(rt.peak_envelope(x.to(DEV), torch.tensor(ll), plan4))
        assert env.dtype == np.float32 and env.shape == x.shape
        for b, r in enumerate(rows):
            assert np.array_equal(env[b, :len(r)], lm.envelope_ref(r)), (fs, b, len(r))
            assert not env[b, len(r):].any(), (fs, b)
    # lengths None: the whole row; a NaN sample inside a row counts as absent
    r = rows[5].copy()
    r[700] = np.nan
    env = _np(rt.peak_envelope(torch.from_numpy(r)[None].to(DEV), None, plan4))
    assert np.array_equal(env[0], lm.envelope_ref(r)) and not np.isnan(env).any()
    tp = rt.true_peak(torch.from_numpy(rows[5])[None].to(DEV), None, plan4)
    assert float(tp[0]) == lm.envelope_ref(rows[5]).max()


def _limit(x, env, ll, g, W, gain_in=None, peak=None, meansq=None):
    """rt.limit at the gain g: level g at mean square 1"""
    from matcha_hip import runtime as rt
    B = x.shape[0]
    peak = torch.ones(B, dtype=torch.float32, device=DEV) if peak is None else peak
    meansq = torch.ones(B, dtype=torch.float64, device=DEV) if meansq is None else meansq
    lens = None if ll is None else torch.tensor(ll, dtype=torch.int32)
    return rt.limit(x.to(DEV), env.to(DEV), lens, (peak, meansq), float(g), C, W, gain_in=gain_in)


@pytest.mark.parametrize("W", (1, 2, 80, 2048))
def test_limit_matches_the_specification(W):
    from matcha_hip import runtime as rt
    T = rt.LIMIT_TILE
    g = np.float32(1.7)
    n = 2 * T + W + 300  # three or four tiles; tile 1 is [T, 2T), its halo [T - (W - 1), 2T + W - 1)
    spots = ([0, n - 1, T - 1, T + W - 1], [T, T - (W - 1), 2 * T + W - 2], [2 * T - 1, 2 * T])
    envs, xs = [], []
    for i, where in enumerate(spots):  # single peaks on a quiet floor
        e = np.full(n, 0.01, dtype=np.float32)
        for j, k in enumerate(where):
            e[k] = 1.0 + 0.5 * j
        envs.append(e)
        xs.append(_noise(n, 400 + i, 0.3))
    envs.append(np.abs(_noise(n, 410, 0.5)))            # over the ceiling at a third of the samples
    xs.append(_noise(n, 411, 0.3))
    for m in (W - 1, 5, 1):                             # rows shorter than the window
        if m >= 1:
            envs.append(np.abs(_noise(m, 420 + m, 1.0)) + np.float32(0.3))
            xs.append(_noise(m, 430 + m, 0.3))
    envs.append(np.zeros(0, np.float32))                # an empty row
    xs.append(np.zeros(0, np.float32))
    for fill in (np.nan, 100.0):
        x, ll = _batch(xs, L=n + 37, fill=fill)
        e, _ = _batch(envs, L=n + 37, fill=fill)
        y, gain, red = (_np(t) for t in _limit(x, e, ll, g, W))
        assert y.dtype == np.float32 and y.shape == x.shape
        for b, (xr, er) in enumerate(zip(xs, envs)):
            m = len(xr)
            s = lm.gain_curve_ref(er, g, C32, W)
            assert np.array_equal(y[b, :m], lm.apply_ref(xr, g, s)), (W, b, m)
            assert not y[b, m:].any() and gain[b] == g, (W, b)
            assert red[b] == (s.min() if m else 1.0), (W, b)
            if m:
                assert (s <= lm.quotient_ref(er, g, C32)).all()
        assert red[3] < 0.5 and red[0] < 1.0


def test_limit_forms_the_gain_on_the_device():
    n, W = 3000, 80
    xs = [_noise(n, 500 + i, 0.3) for i in range(4)]
    envs = [np.abs(_noise(n, 510 + i, 0.4)) for i in range(4)]
    x, ll = _batch(xs)
    e, _ = _batch(envs)
    peak = torch.tensor([0.7, 0.0, 2.0, 0.3], dtype=torch.float32, device=DEV)       # row 1 is not levelled
    meansq = torch.tensor([0.013, 0.5, 0.0, 1e-4], dtype=torch.float64, device=DEV)  # row 2 keeps its gain
    gin = torch.tensor([1.25, 1.0, 3.5, 0.8], dtype=torch.float32, device=DEV)
    level = ld.target_level(-16.0)
    for gain_in in (None, gin):
        y, gain, red = (_np(t) for t in _limit(x, e, ll, level, W, gain_in=gain_in, peak=peak, meansq=meansq))
        for b in range(4):
            g0 = np.float32(1.0) if gain_in is None else _np(gin)[b]
            want = lm.next_gain_ref(g0, level, float(meansq[b])) if float(peak[b]) > 0 else g0
            assert gain[b] == want, (b, gain[b], want)
            s = lm.gain_curve_ref(envs[b], want, C32, W) if float(peak[b]) > 0 else np.ones(n, np.float32)
            assert np.array_equal(y[b], lm.apply_ref(xs[b], want, s)) and red[b] == s.min(), b
    assert lm.next_gain_ref(np.float32(1.0), level, 0.013) == ao.gain_ref(0.7, 0.013, "rms", level, False)


def test_division_is_the_ieee_quotient():
    """W = 1 and a <= 128 c: s = floor(r 2^30) / 2^30 = r, the fp32 quotient itself, on 10^5 random a"""
    rng = np.random.default_rng(7)
    n = 100000
    a = (C * np.exp(rng.uniform(0.0, math.log(100.0), n))).astype(np.float32)
    a[:4] = [np.nextafter(C32, np.float32(2)), C32, np.nextafter(C32, np.float32(0)), np.float32(100.0) * C32]
    x = np.ones(n, dtype=np.float32)
    y, gain, red = (_np(t) for t in _limit(torch.from_numpy(x)[None], torch.from_numpy(a)[None], None, 1.0, 1))
    over = a > C32
    want = np.where(over, C32 / a, np.float32(1.0)).astype(np.float32)
    assert over.sum() > n - 10 and gain[0] == 1.0
    assert np.array_equal(y[0], want)
    assert np.array_equal(y[0], lm.gain_curve_ref(a, 1.0, C32, 1)) and red[0] == want.min()


def _stage(fs, enc="f32", target=-16.0, **kw):
    from hifigan.output import AudioOutput
    return AudioOutput(fs, source_rate=fs, loudness=target, true_peak=CEIL_DB, limiter=5.0, encoding=enc, **kw)


def test_rows_do_not_depend_on_the_batch():
    from matcha_hip import runtime as rt
    fs = 22050
    T = rt.LIMIT_TILE
    lens = [2 * T + 777, 1, 0, 4 * ld.hop_of(fs) + 5, 3001]
    base = [burst_signal(fs, 60 + i, 1.0)[:n] * np.float32(3.0) for i, n in enumerate(lens)]
    stages = {enc: _stage(fs, enc, target=-14.0) for enc in ao.ENCODINGS}

    def run(x, ll):
        lim = stages["f32"].limited(x, ll)
        return lim, {enc: st.finish(x, ll) for enc, st in stages.items()}

    singles = {b: run(torch.from_numpy(r)[None].to(DEV), torch.tensor([len(r)], dtype=torch.int32, device=DEV))
               for b, r in enumerate(base) if len(r)}
    assert float(singles[0][0].reduction[0]) < 1.0 and float(singles[0][0].trim[0]) <= 1.0
    for L, perm in ((max(lens), [0, 1, 2, 3, 4]), (max(lens) + 1234, [3, 2, 4, 0, 1])):
        x, ll = _batch([base[b] for b in perm], L=L, fill=7.0)
        lim, outs = run(x.to(DEV), torch.tensor(ll, dtype=torch.int32, device=DEV))
        for row, b in enumerate(perm):
            n = lens[b]
            if n == 0:
                assert float(lim.gain[row]) == 1 and float(lim.reduction[row]) == 1 and float(lim.trim[row]) == 1
                assert not lim.audio[row].any() and float(outs["f32"].gain[row]) == 1
                continue
            lim1, outs1 = singles[b]
            assert torch.equal(lim.audio[row, :n], lim1.audio[0]) and not lim.audio[row, n:].any(), (L, b)
            for f in ("gain", "reduction", "trim"):
                assert torch.equal(getattr(lim, f)[row], getattr(lim1, f)[0]), (L, b, f)
            for enc in ao.ENCODINGS:
                assert torch.equal(outs[enc].audio[row, :n], outs1[enc].audio[0]), (L, b, enc)
                assert torch.equal(outs[enc].gain[row], outs1[enc].gain[0]), (L, b, enc)


@pytest.mark.parametrize("fs", RATES)
def test_stage_equals_the_specification(fs):
    from hifigan.output import Limited
    x = burst_signal(fs)
    y, g, red, trim, d, _ = _limiter_ref(x, fs, -16.0)
    xd = torch.from_numpy(x)[None].to(DEV)
    ll = torch.tensor([len(x)], dtype=torch.int32, device=DEV)
    lim = _stage(fs).limited(xd, ll)
    assert isinstance(lim, Limited) and lim.sample_rate == fs and torch.equal(lim.lengths, ll)
    print(f"{fs} Hz: gain {float(lim.gain[0]):.5f} (spec {g:.5f}), reduction {float(lim.reduction[0]):.5f}, "
          f"trim {float(lim.trim[0]):.7f}")
    assert np.array_equal(_np(lim.audio)[0], y)
    assert _np(lim.gain)[0] == g and _np(lim.reduction)[0] == red and _np(lim.trim)[0] == trim
    assert red < 1.0 and trim <= 1.0
    q = ao.pcm16_ref(y, trim)
    want = {"f32": d, "pcm16": q, "mulaw": ao.mulaw_ref(q)}
    for enc in ao.ENCODINGS:
        out = _stage(fs, enc)(xd)
        assert out.sample_rate == fs and torch.equal(out.lengths, ll)
        assert np.array_equal(_np(out.audio)[0], want[enc]), (fs, enc)
        assert _np(out.gain)[0] == g * trim, (fs, enc)  # one fp32 product


@pytest.mark.parametrize("fs", RATES)
def test_delivered_true_peak_is_at_or_under_the_ceiling(fs):
    """mt_true_peak of the f32 output against c = 10^(-1/20), with no margin: the trim carries the headroom
    (limiter.trim_headroom, 6.4e-6 at this filter) that the fp32 product trim * y and the meter's FMA chain can add."""
    from hifigan.output import AudioOutput
    from matcha_hip import runtime as rt
    x = burst_signal(fs)
    out = _stage(fs)(torch.from_numpy(x)[None].to(DEV))
    tp = float(rt.true_peak(out.audio, out.lengths, rt.resample_plan(fs, 4 * fs))[0])
    d = _limiter_ref(x, fs, -16.0)[4]
    print(f"{fs} Hz: delivered true peak / c - 1 = {tp / C - 1.0:+.2e}")
    assert tp == ld.true_peak_ref(d) and tp >= C * (1.0 - 2.0 * lm.default_headroom())
    m = AudioOutput(fs, source_rate=fs).measure(out.audio)
    assert abs(float(m.true_peak_db[0]) - 20.0 * math.log10(tp)) < 1e-12
    assert tp <= C


@pytest.mark.parametrize("fs", RATES)
def test_rows_that_need_no_limiting_keep_todays_bytes(fs):
    from hifigan.output import AudioOutput
    x = _noise(3 * fs, 90, 0.05)
    target = -26.0
    # on the CPU first: at the gain to the target the envelope stays 3 dB clear of the ceiling
    E, _ = ld.loudness_ref(x, fs)
    g = ld.loudness_gain_ref(E, ld.true_peak_ref(x), target, CEIL_DB, limit=False)
    assert float((g * lm.envelope_ref(x)).max()) < C * 10.0 ** (-3.0 / 20.0)
    xd = torch.from_numpy(x)[None].to(DEV)
    lim = _stage(fs, target=target).limited(xd, torch.tensor([len(x)], dtype=torch.int32, device=DEV))
    assert float(lim.reduction[0]) == 1.0 and float(lim.trim[0]) == 1.0
    for enc in ao.ENCODINGS:
        today = AudioOutput(fs, source_rate=fs, loudness=target, true_peak=CEIL_DB, encoding=enc)(xd)
        new = _stage(fs, enc, target=target)(xd)
        assert torch.equal(new.audio, today.audio) and torch.equal(new.gain, today.gain), (fs, enc)


@pytest.mark.parametrize("fs", RATES)
def test_the_limiter_delivers_the_loudness_the_cap_gives_up(fs):
    from hifigan.output import AudioOutput
    x = burst_signal(fs)
    xd = torch.from_numpy(x)[None].to(DEV)
    meter = AudioOutput(fs, source_rate=fs)
    capped = AudioOutput(fs, source_rate=fs, loudness=-16.0, true_peak=CEIL_DB)(xd)
    limited = _stage(fs)(xd)
    l_cap, l_lim = float(meter.measure(capped.audio).lufs[0]), float(meter.measure(limited.audio).lufs[0])
    d, want = _limiter_ref(x, fs, -16.0)[4:6]
    print(f"{fs} Hz: capped {l_cap:.3f} LUFS, limited {l_lim:.3f} LUFS (specification {want:.3f}), target -16")
    assert np.array_equal(_np(limited.audio)[0], d)
    assert l_cap < l_lim < -16.0 + 0.5 and abs(l_lim + 16.0) < abs(l_cap + 16.0)
    assert abs(l_lim - want) <= 1e-9


# ---- LongForm -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tts():
    """test_gpu_join.py's models: the smallest of the conftest factories on synthetic weights, two documents of three
    short sentences"""
    from hifigan.denoiser import Denoiser
    from matcha_hip import synthetic
    m = make_matcha(1)
    sd = synthetic.make_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 1,
                                   force_log_duration=math.log(1.5))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to(DEV).eval()
    g = make_generator("fp32")
    gsd = synthetic.make_state_dict([(k, tuple(v.shape)) for k, v in g.state_dict().items()], 2)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in gsd.items()})
    g = g.to(DEV).eval()
    g.remove_weight_norm()
    den = Denoiser(g, mode="zeros")
    x, xl = synthetic.synthetic_text(6, seed=3, lo=9, hi=15)
    sents = [torch.from_numpy(x[i, :xl[i]].copy()).to(DEV) for i in range(6)]
    return dict(m=m, g=g, den=den, docs=[sents[:3], sents[3:]], seeds=[11, 12])


def test_longform_limits_whole_documents(tts):
    from hifigan.longform import LongForm
    from hifigan.output import AudioOutput
    fs, target = 16000, -9.0  # the noise-like output of synthetic weights has a low crest: a high target engages the limiter
    output = AudioOutput(fs, loudness=target, true_peak=CEIL_DB, limiter=5.0, encoding="pcm16")
    lf = LongForm(tts["m"], tts["g"], tts["den"], output, n_timesteps=2, pause_ms=12.0, fade_ms=2.0, head_ms=1.0,
                  tail_ms=3.0, trim_pad_ms=1.0, trim_db=None)
    seg, lens, doc_first = lf.segments(tts["docs"], seeds=tts["seeds"])
    assert seg.shape[0] == 6 and doc_first.tolist() == [0, 3, 6]
    doc = lf(tts["docs"], seeds=tts["seeds"])
    seg_np, lens_np = _np(seg), _np(lens)
    gap = lf._gaps(None, [0, 3, 6])
    dst, doc_len, bad = jn.plan_ref([0, 3, 6], [0] * 6, lens_np, gap, lf.head, lf.tail, seg.shape[1])
    assert bad == 0 and np.array_equal(_np(doc.lengths), doc_len)
    joined = jn.join_ref(seg_np, [0] * 6, lens_np, [0, 3, 6], dst, doc_len, lf.fade)
    for d in range(2):
        n = int(doc_len[d])
        y, g, red, trim = lm.limiter_ref(joined[d, :n], fs, target, CEIL_DB, 80, 3)
        print(f"document {d}: {n} samples, gain {g:.4f}, reduction {red:.4f}, trim {trim:.6f}")
        assert red < 1.0
        assert np.array_equal(_np(doc.audio)[d, :n], ao.pcm16_ref(y, trim)), d
        assert not _np(doc.audio)[d, n:].any() and _np(doc.gain)[d] == g * trim, d
