"""Loudness and true peak on the GPU (csrc/mt_loudness.hip): mt_loudness, mt_true_peak and the
`loudness=` path of hifigan.output.AudioOutput against the CPU specification matcha_hip/loudness.py.

  - block energies z within 1e-9 relative of the sequential fp64 filter (the bar §19 sets for meansq; the chunked scan
    itself sits near 1e-13), block counts exact, with row ends at the block rules' edges, around the scan's tile and
    inside a chunk that a hop boundary splits;
  - the gated energy BIT-EQUAL to the specification's gating applied to the GPU's own z (the gating is plain fp64
    operations in block order on both sides), on inputs whose blocks the CPU first shows to lie clear of both gates;
  - the true peak bit-equal to the peaks of the signal and of the resampler's own 4x output, and to the
    specification's fp32 FMA chain;
  - every row of a padded batch equal to its one-utterance call, bit for bit;
  - the stage: gain bit-equal to loudness_gain_ref of the GPU's (E, TP), bytes bit-equal to the encoders'
    references, the delivered loudness on target, the true-peak ceiling kept.
"""
import math

import numpy as np
import pytest
import torch

from conftest import make_generator

from matcha_hip import audio_out as ao
from matcha_hip import loudness as ld

pytestmark = pytest.mark.gpu
DEV = "cuda"
RATES = (8000, 22050)


def _noise(n, seed, scale=0.1):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)


def three_level(fs=8000, seed=0):
    """1 s of N(0,1) * 0.1, 1 s at 25 dB below that, 0.5 s at 1e-5"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(fs) * 0.1
    b = rng.standard_normal(fs) * 0.1 * 10.0 ** (-25.0 / 20.0)
    c = rng.standard_normal(fs // 2) * 1e-5
    return np.concatenate([a, b, c]).astype(np.float32)


def _batch(rows, L=None, fill_seed=None):
    """rows: list of fp32 arrays -> (x [B, L] host, lens); the padding holds noise when fill_seed is given"""
    L = max(max(len(r) for r in rows), 1) if L is None else L
    x = np.zeros((len(rows), L), dtype=np.float32) if fill_seed is None else _noise(len(rows) * L, fill_seed,
                                                                                    0.5).reshape(len(rows), L)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    return torch.from_numpy(x), [len(r) for r in rows]


_REF = {}


def _ref(x, fs):
    """(E, z) of the specification, computed once per (row, rate)"""
    key = (x.tobytes(), fs)
    if key not in _REF:
        _REF[key] = ld.loudness_ref(x, fs)
    return _REF[key]


@pytest.mark.parametrize("fs", RATES)
def test_block_energies_and_counts(fs):
    from matcha_hip import runtime as rt
    h, T, C = ld.hop_of(fs), rt.LOUDNESS_TILE, rt.LOUDNESS_CHUNK
    # the block rules' edges; the scan's tile - 1, tile, tile + 1 and two tiles + 1; and a row that ends two samples
    # past a hop boundary k h which falls inside a chunk, so that the chunk's two partials both count (at 22,050 Hz,
    # h = 2205 = 68 * 32 + 29; at 8000 Hz every boundary is a chunk's first sample, h = 25 * 32: the unsplit path)
    lens = [0, 1, 4 * h - 1, 4 * h, 5 * h - 1, 5 * h, T - 1, T, T + 1, 2 * T + 1]
    k = next((k for k in range(5, 40) if 0 < (k * h) % C < C - 2), None)
    assert (k is None) == (h % C == 0) == (fs == 8000)
    if k is not None:
        assert (k * h) // C == (k * h + 2) // C
        lens.append(k * h + 2)
    groups = [lens[:6], lens[6:]]
    worst = 0.0
    for gi, group in enumerate(groups):
        rows = [_noise(n, 100 + gi * 16 + i) for i, n in enumerate(group)]
        x, ll = _batch(rows, fill_seed=7 + gi)
        E, nb, z = rt.loudness(x.to(DEV), torch.tensor(ll), fs, return_blocks=True)
        assert E.dtype == torch.float64 and nb.dtype == torch.int32 and z.dtype == torch.float64
        assert z.shape == (len(rows), max(ld.block_count(x.shape[1], fs), 1))
        E, nb, z = E.cpu().numpy(), nb.cpu().tolist(), z.cpu().numpy()
        for b, r in enumerate(rows):
            Er, zr = _ref(r, fs)
            J = ld.block_count(len(r), fs)
            assert nb[b] == J == zr.shape[0], (fs, len(r), nb[b], J)
            assert not z[b, J:].any()
            if J == 0:
                assert E[b] == 0.0
                continue
            err = np.abs(z[b, :J] / zr - 1.0).max()
            worst = max(worst, err)
            assert err <= 1e-9, (fs, len(r), err)
            assert E[b] == ld.gate_ref(z[b, :J]), (fs, len(r))
            assert abs(E[b] - Er) <= 1e-9 * Er, (fs, len(r))
    print(f"{fs} Hz: worst relative error of a block energy {worst:.1e}")


def test_gating_is_the_specifications_bit_for_bit():
    from matcha_hip import runtime as rt
    fs = 8000
    rows = [three_level(fs, 0), three_level(fs, 1)[::-1].copy(), _noise(3 * fs, 5, 1e-5), np.zeros(2 * fs, np.float32)]
    # on the CPU first: no block of these rows lies within 0.1 LU of either gate
    for r in rows[:2]:
        E, z = _ref(r, fs)
        m1 = z > ld.ABS_GATE
        lz = 10.0 * np.log10(z)
        assert np.abs(lz - 10.0 * math.log10(ld.ABS_GATE)).min() > 0.1
        assert np.abs(lz - 10.0 * math.log10(0.1 * z[m1].mean())).min() > 0.1
    assert ld.gate_counts(_ref(rows[0], fs)[1]) == (22, 20, 10)
    assert ld.gate_counts(_ref(rows[2], fs)[1]) == (27, 0, 0)  # all under the absolute gate
    x, ll = _batch(rows, fill_seed=3)
    E, nb, z = rt.loudness(x.to(DEV), torch.tensor(ll), fs, return_blocks=True)
    E, nb, z = E.cpu().numpy(), nb.cpu().tolist(), z.cpu().numpy()
    for b, r in enumerate(rows):
        Er, zr = _ref(r, fs)
        assert nb[b] == zr.shape[0]
        assert E[b] == ld.gate_ref(z[b, :nb[b]]), b            # bit for bit on the GPU's own blocks
        assert ld.gate_counts(z[b, :nb[b]]) == ld.gate_counts(zr), b
        assert abs(E[b] - Er) <= 1e-9 * Er, (b, E[b], Er)
    assert E[2] == 0.0 and E[3] == 0.0
    print(f"three-level row: {ld.lufs(E[0]):.3f} LUFS gated, {ld.lufs(z[0, :nb[0]].mean()):.3f} ungated")


def test_true_peak_is_the_resamplers_peak():
    from matcha_hip import runtime as rt
    fs = 8000
    plan4 = rt.resample_plan(fs, 4 * fs)
    assert (plan4.up, plan4.down, plan4.half) == (4, 1, 40)
    lens = [1, 511, 512, 513, 2049, 0]  # 4 n outputs: 2044, 2048, 2052 and 8196 around the 2048-output tiles
    rows = [_noise(n, 40 + i, 0.4) for i, n in enumerate(lens)]
    # the unit sine at fs / 4, 45 degrees, faded in and out: samples of +-0.7071 under an inter-sample peak of 1
    w = np.ones(2049)
    w[:256] = 0.5 - 0.5 * np.cos(np.pi * np.arange(256) / 256)
    w[-256:] = w[:256][::-1]
    rows[4] = (np.sin(2.0 * np.pi * 0.25 * np.arange(2049) + np.pi / 4.0) * w).astype(np.float32)
    x, ll = _batch(rows, fill_seed=9)
    xd, ld_ = x.to(DEV), torch.tensor(ll, device=DEV)
    tp = rt.true_peak(xd, ld_, plan4)
    assert tp.dtype == torch.float32 and tp.shape == (len(rows),)
    y, ol = rt.resample(xd, plan4, ld_)
    want = torch.maximum(rt.audio_stats(xd, ld_)[0], rt.audio_stats(y, ol)[0])
    assert torch.equal(tp, want), (tp, want)
    tp = tp.cpu().numpy()
    for b, r in enumerate(rows):
        assert tp[b] == ld.true_peak_ref(r), (b, tp[b], ld.true_peak_ref(r))  # the specification's fp32 FMA chain
    assert tp[5] == 0.0
    assert abs(np.abs(rows[4]).max() - 0.7071) < 1e-4 and abs(20 * math.log10(tp[4])) <= 0.05
    # unit impulses: the largest fp32 tap exactly (at half scale, so that the sample itself is not the peak)
    taps = plan4.h.astype(np.float32)
    imp = np.zeros((3, 700), dtype=np.float32)
    for b, k0 in enumerate((0, 350, 699)):
        imp[b, k0] = 0.5
    got = rt.true_peak(torch.from_numpy(imp).to(DEV), None, plan4).cpu().numpy()
    assert taps.argmax() == 40 and taps.max() > 1.0  # the centre tap, 1.0006366
    assert (got == max(np.float32(0.5), np.float32(0.5) * taps.max())).all(), (got, taps.max())
    one = np.zeros((1, 700), dtype=np.float32)
    one[0, 123] = 1.0
    assert float(rt.true_peak(torch.from_numpy(one).to(DEV), None, plan4)[0]) == max(np.float32(1.0), taps.max())


def _measure_and_encode(x, lens, fs, plan4, target, ceiling, limit):
    from matcha_hip import runtime as rt
    E, nb, z = rt.loudness(x, lens, fs, return_blocks=True)
    tp = rt.true_peak(x, lens, plan4)
    peak_eff = (tp.double() / 10.0 ** (ceiling / 20.0)).float()
    peak_eff = torch.where(E > 0, peak_eff, torch.zeros_like(peak_eff))
    outs = {}
    for enc in ao.ENCODINGS:
        outs[enc], gain = rt.encode_audio(x, lens, "rms", ld.target_level(target), limit, enc, stats=(peak_eff, E))
    return E, nb, z, tp, gain, outs


def test_rows_do_not_depend_on_the_batch():
    from matcha_hip import runtime as rt
    fs = 22050
    plan4 = rt.resample_plan(fs, 4 * fs)
    T = rt.LOUDNESS_TILE
    lens = [2 * T + 777, 1, 0, 4 * ld.hop_of(fs) + 5, 3001]
    base = [_noise(n, 60 + i, 0.2) for i, n in enumerate(lens)]
    singles = {}
    for b, r in enumerate(base):
        if len(r):
            singles[b] = _measure_and_encode(torch.from_numpy(r)[None].to(DEV), None, fs, plan4, -14.0, -1.0, True)
    assert float(singles[0][4][0]) != 1.0
    for L, perm in ((lens[0], [0, 1, 2, 3, 4]), (lens[0] + 1234, [3, 2, 4, 0, 1])):
        x, ll = _batch([base[b] for b in perm], L=L, fill_seed=L)
        E, nb, z, tp, gain, outs = _measure_and_encode(x.to(DEV), torch.tensor(ll, device=DEV), fs, plan4, -14.0,
                                                       -1.0, True)
        for row, b in enumerate(perm):
            n = lens[b]
            if n == 0:
                assert float(E[row]) == 0 and int(nb[row]) == 0 and float(tp[row]) == 0 and float(gain[row]) == 1
                assert not z[row].any()
                continue
            E1, nb1, z1, tp1, gain1, outs1 = singles[b]
            J = int(nb1[0])
            assert int(nb[row]) == J and torch.equal(z[row, :J], z1[0, :J]) and not z[row, J:].any(), (L, b)
            assert torch.equal(E[row], E1[0]) and torch.equal(tp[row], tp1[0]), (L, b)
            assert torch.equal(gain[row], gain1[0]), (L, b)
            for enc in ao.ENCODINGS:
                assert torch.equal(outs[enc][row, :n], outs1[enc][0]), (L, b, enc)


def test_stage_levels_to_the_target():
    from hifigan.output import AudioOutput
    from matcha_hip import runtime as rt
    src = three_level(22050, 0)
    x = torch.from_numpy(src)[None].to(DEV)
    plan = rt.resample_plan(22050, 16000)
    plan4 = rt.resample_plan(16000, 64000)
    y, ol = rt.resample(x, plan)
    E, _ = rt.loudness(y, ol, 16000)
    tp = rt.true_peak(y, ol, plan4)
    want = ld.loudness_gain_ref(float(E[0]), tp[0].cpu().numpy(), -16.0, -1.0, True)
    yh = y[0].cpu().numpy()
    outs = {}
    for enc in ao.ENCODINGS:
        stage = AudioOutput(16000, source_rate=22050, loudness=-16, encoding=enc, hop=1)
        outs[enc] = out = stage(x)
        assert out.sample_rate == 16000 and torch.equal(out.lengths, ol)
        assert out.gain.cpu().numpy()[0] == want, (enc, out.gain, want)
    q = ao.pcm16_ref(yh, want)
    assert np.array_equal(outs["pcm16"].audio[0].cpu().numpy(), q)
    assert np.array_equal(outs["mulaw"].audio[0].cpu().numpy(), ao.mulaw_ref(q))
    assert np.array_equal(outs["f32"].audio[0].cpu().numpy(), ao.f32_ref(yh, want))
    # the delivered signal reads the target: the fp32 gain and product move it by about 1e-6 LU
    m = AudioOutput(16000, source_rate=16000).measure(outs["f32"].audio)
    assert m.sample_rate == 16000 and m.lufs.dtype == torch.float64 and m.true_peak_db.dtype == torch.float64
    print(f"delivered {float(m.lufs[0]):.6f} LUFS, {float(m.true_peak_db[0]):.3f} dBTP, gain {float(want):.4f}")
    assert abs(float(m.lufs[0]) - (-16.0)) <= 1e-3
    # measure() reads the resampled signal at gain 1, whether or not loudness= is set
    for st in (AudioOutput(16000, source_rate=22050, hop=1), AudioOutput(16000, source_rate=22050, loudness=-23, hop=1)):
        m0 = st.measure(x)
        assert abs(float(m0.lufs[0]) - ld.lufs(float(E[0]))) < 1e-12
        assert abs(float(m0.true_peak_db[0]) - 20.0 * math.log10(float(tp[0]))) < 1e-12
        assert torch.equal(m0.lengths, ol)


def test_stage_keeps_the_true_peak_ceiling():
    from hifigan.output import AudioOutput
    fs = 16000
    x = torch.from_numpy(_noise(3 * fs, 77, 0.1))[None].to(DEV)  # Gaussian noise: -3 LUFS would need peaks far past 1
    capped = AudioOutput(fs, source_rate=fs, loudness=-3.0, true_peak=-1.0)(x)
    free = AudioOutput(fs, source_rate=fs, loudness=-3.0, true_peak=-1.0, limit=False)(x)
    m_in = AudioOutput(fs, source_rate=fs).measure(x)
    E = 10.0 ** ((float(m_in.lufs[0]) + 0.691) / 10.0)
    uncapped = ld.target_level(-3.0) / math.sqrt(E)
    assert abs(float(free.gain[0]) / uncapped - 1.0) < 1e-6  # limit=False reproduces the uncapped gain
    assert float(capped.gain[0]) < float(free.gain[0])
    m = AudioOutput(fs, source_rate=fs).measure(capped.audio)
    tp_out = 10.0 ** (float(m.true_peak_db[0]) / 20.0)
    print(f"gain {float(capped.gain[0]):.4f} (uncapped {uncapped:.4f}), delivered true peak {tp_out:.7f}")
    assert tp_out <= 10.0 ** (-1.0 / 20.0) * (1 + 2.0 ** -22)
    assert float(capped.audio.abs().max()) < 1.0      # no sample at +-1: the encoder's clamp never worked
    assert float(free.audio.abs().max()) == 1.0       # ... as it does without the limit
    assert float(m.lufs[0]) < -3.0


def test_measure_on_the_vocoders_output():
    from hifigan.denoiser import Denoiser
    from hifigan.output import AudioOutput
    from matcha_hip import runtime as rt
    from matcha_hip import synthetic
    g = make_generator("bf16")
    sd = synthetic.make_state_dict([(k, tuple(v.shape)) for k, v in g.state_dict().items()], 8)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    g = g.to(DEV).eval()
    g.remove_weight_norm()
    den = Denoiser(g, mode="zeros")
    B, T = 2, 40
    lens = torch.tensor([40, 33], device=DEV)
    mel = (torch.randn(B, 80, T, generator=torch.Generator().manual_seed(11)) * 2.1 - 5.5).to(DEV)
    d = den(g(mel, lengths=lens).squeeze(1), strength=0.00025, lengths=lens)
    stage = AudioOutput(16000, loudness=-16)
    m = stage.measure(d, lens)
    y, ol = rt.resample(d, rt.resample_plan(22050, 16000), lens, lmul=256)
    peak, _ = rt.audio_stats(y, ol)
    assert torch.equal(m.lengths, ol) and m.lengths.cpu().tolist() == [ao.out_length(256 * n, 320, 441) for n in (40, 33)]
    assert bool(torch.isfinite(m.lufs).all()) and bool(torch.isfinite(m.true_peak_db).all())
    assert bool((m.true_peak_db >= 20.0 * torch.log10(peak.double())).all())
    out = stage(d, lens)
    assert out.audio.shape == y.shape and bool(torch.isfinite(out.gain).all()) and torch.equal(out.lengths, ol)
    print(f"lufs {m.lufs.cpu().tolist()}, dBTP {m.true_peak_db.cpu().tolist()}, gain {out.gain.cpu().tolist()}")


def test_wave_streamer_refuses_loudness():
    from hifigan.denoiser import Denoiser
    from hifigan.output import AudioOutput
    from hifigan.stream import WaveStreamer
    g = make_generator("bf16").to(DEV).eval()
    g.remove_weight_norm()
    den = Denoiser(g, mode="zeros")
    with pytest.raises(ValueError, match="loudness"):
        WaveStreamer(g, den, AudioOutput(16000, loudness=-16))
