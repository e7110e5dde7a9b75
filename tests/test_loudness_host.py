"""Loudness and true peak, host side (CPU only: no kernel launches): the specification in matcha_hip/loudness.py
 against ITU-R BS.1770-4's coefficient table, scipy's lfilter, the EBU Tech 3341 conformance sine and
its own block / gating rules, and the argument checks of the C ABI and of AudioOutput."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO

from matcha_hip import audio_out as ao
from matcha_hip import loudness as ld

# BS.1770-4, table 1 and table 2 (48 kHz)
STAGE1_B = (1.53512485958697, -2.69169618940638, 1.19839281085285)
STAGE1_A = (1.0, -1.69065929318241, 0.73248077421585)
STAGE2_B = (1.0, -2.0, 1.0)
STAGE2_A = (1.0, -1.99004745483398, 0.99007225036621)


def three_level(fs=8000, seed=0):
    """1 s of N(0,1) * 0.1, 1 s at 25 dB below that, 0.5 s at 1e-5"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(fs) * 0.1
    b = rng.standard_normal(fs) * 0.1 * 10.0 ** (-25.0 / 20.0)
    c = rng.standard_normal(fs // 2) * 1e-5
    return np.concatenate([a, b, c]).astype(np.float32)


def quarter_rate_sine(n, fade=256):
    """the unit sine at fs / 4 with phase 45 degrees: every sample is +-0.7071, the waveform between them reaches 1.
    Faded in and out over `fade` samples (raised cosine): switched on at full level it would be another signal, whose
    onset step overshoots to +0.115 dBTP on its own."""
    x = np.sin(2.0 * np.pi * 0.25 * np.arange(n) + np.pi / 4.0)
    w = 0.5 - 0.5 * np.cos(np.pi * np.arange(fade) / fade)
    x[:fade] *= w
    x[n - fade:] *= w[::-1]
    return x.astype(np.float32)


def test_coefficients_at_48k_are_the_standards_table():
    b1, a1, b2, a2 = ld.k_weighting(48000)
    worst = max(np.abs(b1 - STAGE1_B).max(), np.abs(a1 - STAGE1_A).max(), np.abs(b2 - STAGE2_B).max(),
                np.abs(a2 - STAGE2_A).max())
    print(f"48 kHz coefficients against the table: {worst:.1e}")
    assert worst <= 1e-12
    c = ld.coefficients(48000)
    assert c.shape == (10,) and c.dtype == np.float64
    assert c.tolist() == [*b1, a1[1], a1[2], *b2, a2[1], a2[2]]
    assert ld.hop_of(48000) == 4800 and ld.hop_of(22050) == 2205 and ld.hop_of(8000) == 800 and ld.hop_of(11025) == 1103
    with pytest.raises(ValueError):
        ld.k_weighting(7999)


def test_filter_against_scipy_lfilter_stage_by_stage():
    pytest.importorskip("scipy")
    from scipy import signal
    x = np.random.default_rng(1).standard_normal(4000)
    for fs in (8000, 22050, 48000):
        b1, a1, b2, a2 = ld.k_weighting(fs)
        y1, y2 = ld.biquad_ref(b1, a1, x), ld.biquad_ref(b2, a2, x)  # each stage on the unit noise itself
        e1 = np.abs(y1 - signal.lfilter(b1, a1, x)).max()
        e2 = np.abs(y2 - signal.lfilter(b2, a2, x)).max()
        print(f"{fs}: stage 1 {e1:.1e}, stage 2 {e2:.1e}")
        assert e1 <= 1e-12 and e2 <= 1e-12, (fs, e1, e2)
        y2 = ld.biquad_ref(b2, a2, y1)
        assert np.abs(y2 - signal.lfilter(b2, a2, signal.lfilter(b1, a1, x))).max() <= 1e-12
        assert np.array_equal(ld.k_filter_ref(x, fs), y2)


@pytest.mark.parametrize("fs", [8000, 16000, 22050, 44100, 48000])
def test_conformance_sine(fs):
    """997 Hz, full scale, 2 s: -3.01 LUFS within EBU Tech 3341's +-0.1 LU"""
    x = np.sin(2.0 * np.pi * 997.0 * np.arange(2 * fs) / fs).astype(np.float32)
    E, z = ld.loudness_ref(x, fs)
    got = ld.lufs(E)
    print(f"{fs} Hz: {got:.4f} LUFS over {z.shape[0]} blocks")
    assert z.shape[0] == 17
    assert abs(got - (-3.01)) <= 0.1, (fs, got)


def test_gating_on_the_three_level_signal():
    fs = 8000
    x = three_level(fs)
    E, z = ld.loudness_ref(x, fs)
    assert ld.gate_counts(z) == (22, 20, 10)
    gated, ungated = ld.lufs(E), ld.lufs(z.mean())
    print(f"gated {gated:.2f} LUFS, ungated {ungated:.2f} LUFS")
    assert gated > ungated + 3.0
    assert abs(gated - (-18.46)) < 0.01 and abs(ungated - (-21.87)) < 0.01
    # the decisions in numpy's words
    m1 = z > ld.ABS_GATE
    m2 = m1 & (z > 0.1 * z[m1].mean())
    assert E == pytest.approx(z[m2].mean(), rel=1e-14)
    # no block within 0.1 LU of a gate: a decision cannot flip inside a tolerance (the GPU tests rely on this)
    lz = 10.0 * np.log10(z)
    rel = 10.0 * math.log10(0.1 * z[m1].mean())
    assert np.abs(lz - 10.0 * math.log10(ld.ABS_GATE)).min() > 0.1 and np.abs(lz - rel).min() > 0.1


def test_block_edge_rules():
    fs = 8000
    h = ld.hop_of(fs)
    x = (np.random.default_rng(2).standard_normal(5 * h) * 0.1).astype(np.float32)
    for n, J in ((0, 0), (1, 1), (4 * h - 1, 1), (4 * h, 1), (5 * h - 1, 1), (5 * h, 2)):
        z = ld.block_energies(x[:n], fs)
        assert z.shape == (J,) and ld.block_count(n, fs) == J, n
        if n == 0:
            continue
        y2 = ld.k_filter_ref(x[:n], fs) ** 2
        if n < 4 * h:  # one block over the n samples there are
            assert z[0] == pytest.approx(y2.sum() / n, rel=1e-14), n
        else:          # complete blocks only: what follows the last one is not measured
            assert z[0] == pytest.approx(y2[:4 * h].sum() / (4 * h), rel=1e-14), n
        if J == 2:
            assert z[1] == pytest.approx(y2[h:5 * h].sum() / (4 * h), rel=1e-14)
    assert ld.gate_ref(np.zeros(0)) == 0.0
    # a silent row and a row under the absolute gate: E = 0, gain 1
    for row in (np.zeros(3 * fs, dtype=np.float32), (np.random.default_rng(3).standard_normal(3 * fs) * 1e-5)):
        E, z = ld.loudness_ref(row, fs)
        assert z.shape[0] == 27 and E == 0.0 and ld.lufs(E) == -math.inf
        assert ld.loudness_gain_ref(E, ld.true_peak_ref(row), -16.0) == np.float32(1.0)


def test_true_peak_reads_the_inter_sample_peak():
    n = 4000
    x = quarter_rate_sine(n)
    peak = np.abs(x).max()
    tp = ld.true_peak_ref(x)
    print(f"sample peak {peak:.4f} ({20 * math.log10(peak):+.2f} dBFS), true peak {20 * math.log10(tp):+.3f} dBTP")
    assert tp.dtype == np.float32
    assert abs(peak - 0.7071) < 1e-4
    assert abs(20.0 * math.log10(tp)) <= 0.05
    assert ld.true_peak_ref(np.zeros(0)) == 0.0
    # the chain is the resampler's: its fp32 FMA evaluation agrees with the fp64 sum on the same fp32 taps within the
    # forward error bound of the chain, and a unit impulse returns the fp32 taps themselves
    h, half = ao.design_filter(4, 1)
    h32 = h.astype(np.float32)
    r = ld.oversample4_ref(x)
    ref = ao.resample_ref(x, 4, 1, h32.astype(np.float64), half)
    P = np.abs(ao.polyphase(h32, half, 4).astype(np.float64))
    assert r.dtype == np.float32 and r.shape == ref.shape == (4 * n,)
    assert np.abs(r - ref).max() <= (P.shape[1] + 1) * 2.0 ** -24 * P.sum(axis=1).max()
    imp = np.zeros(64, dtype=np.float32)
    imp[20] = 1.0
    assert np.array_equal(ld.oversample4_ref(imp)[80 - half:80 + half + 1], h32)
    assert ld.true_peak_ref(imp) == max(np.float32(1.0), h32.max())


def test_fma32_rounds_once():
    """a b + c = 1 + 2^-23 + 2^-24 - 2^-70 lies just under an fp32 tie: rounding the product-sum to fp64 first lands
    on the tie and then goes to even, 1 + 2^-22; the single rounding of an FMA gives 1 + 2^-23"""
    f = np.float32
    a = np.array([f(2.0 ** -12 * (1 + 2.0 ** -23))])
    b = np.array([f(2.0 ** -12 * (1 - 2.0 ** -23))])
    c = np.array([f(1 + 2.0 ** -23)])
    twice = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f)
    assert twice[0] == f(1 + 2.0 ** -22)
    assert ld._fma32(a, b, c)[0] == f(1 + 2.0 ** -23)
    assert ld._fma32(a, -b, -c)[0] == -f(1 + 2.0 ** -23)
    assert ld._fma32(np.array([f(3.0)]), np.array([f(0.5)]), np.array([f(0.25)]))[0] == f(1.75)  # exact: untouched


def test_loudness_gain_ref():
    E, target = 10.0 ** ((-30.0 + 0.691) / 10.0), -16.0  # a row at -30 LUFS
    # uncapped: +14 dB
    g = ld.loudness_gain_ref(E, 0.1, target)
    assert g.dtype == np.float32 and g == np.float32(ld.target_level(target) / math.sqrt(E))
    assert abs(20 * math.log10(g) - 14.0) < 1e-5
    # capped at the ceiling: g TP <= c (1 + 2^-23)
    c = 10.0 ** (-1.0 / 20.0)
    for TP in (np.float32(0.5), np.float32(0.3333), np.float32(0.97)):
        gc = ld.loudness_gain_ref(E, TP, target, -1.0)
        assert gc < g and float(gc) * float(TP) <= c * (1 + 2.0 ** -23), TP
        assert float(gc) * float(TP) >= c * (1 - 2.0 ** -22), TP
        assert ld.loudness_gain_ref(E, TP, target, -1.0, limit=False) == g
    assert ld.loudness_gain_ref(E, 0.5, target, 0.0) == np.float32(2.0)
    # nothing to level
    assert ld.loudness_gain_ref(0.0, 0.5, target) == np.float32(1.0)
    assert ld.loudness_gain_ref(0.0, 0.0, target) == np.float32(1.0)
    assert ld.effective_peak(0.5, 0.0, -1.0) == 0.0


def test_tile_and_chunk_match_the_kernel():
    from matcha_hip import runtime as rt
    src = open(os.path.join(REPO, "matcha-tts_amd", "csrc", "mt_loudness.hip")).read()
    m = re.search(r"constexpr int KW_CH = (\d+);", src)
    assert m and int(m.group(1)) == rt.LOUDNESS_CHUNK
    m = re.search(r"constexpr int KW_THREADS = (\d+);", src)
    assert m and int(m.group(1)) * rt.LOUDNESS_CHUNK == rt.LOUDNESS_TILE
    m = re.search(r"constexpr int TP_TN = (\d+);", src)
    assert m and int(m.group(1)) == rt.RESAMPLE_TILE


def test_c_abi_refuses_bad_arguments_before_any_launch():
    from matcha_hip import runtime as rt
    L = rt.lib()
    assert L.mt_abi_version() == 1
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused while its arguments are checked
    coef = (ctypes.c_double * 10)(*ld.coefficients(8000).tolist())

    def last():
        return L.mt_last_error().decode()

    def loud(B=1, Ln=4000, hop=800, gate=ld.ABS_GATE, z=None, Jcap=1, ws=p, ws_bytes=1 << 30, coef=coef, audio=p,
             nblocks=p, energy=p):
        return L.mt_loudness(audio, B, Ln, None, coef, hop, gate, z, Jcap, nblocks, energy, ws, ws_bytes, None)

    assert loud(B=0) != 0 and "B 0" in last()
    assert loud(Ln=0) != 0 and "L 0" in last()
    assert loud(Ln=(1 << 30) + 1) != 0 and "loudness: B" in last()
    assert loud(hop=31) != 0 and "hop 31" in last()
    assert loud(hop=(1 << 24) + 1) != 0 and "hop" in last()
    assert loud(audio=None) != 0 and "null argument" in last()
    assert loud(coef=None) != 0 and "null argument" in last()
    assert loud(nblocks=None) != 0 and "null argument" in last()
    assert loud(energy=None) != 0 and "null argument" in last()
    bad = (ctypes.c_double * 10)(*ld.coefficients(8000).tolist())
    bad[4] = float("nan")
    assert loud(coef=bad) != 0 and "coefficient 4" in last()
    for g in (-1.0, float("inf"), float("nan")):
        assert loud(gate=g) != 0 and "absolute gate" in last(), g
    assert loud(Ln=8000, z=p, Jcap=6) != 0 and "Jcap 6 < 7" in last()
    assert loud(Ln=8000, z=p, Jcap=0) != 0 and "Jcap 0" in last()
    assert loud(ws=None) != 0 and "workspace" in last()
    assert loud(ws=ctypes.c_void_p(4104)) != 0 and "16-byte aligned" in last()
    need = L.mt_loudness_workspace_bytes(2, 20000, 800)
    # 3 tiles per row: 4 doubles of state per tile, 2 per chunk of 32 samples, 20000 / 800 + 4 hops, 22 blocks
    assert need == 2 * 8 * (3 * 4 + 3 * 256 * 2 + 29 + 22)
    assert loud(B=2, Ln=20000, ws_bytes=need - 1) != 0 and "workspace too small" in last()
    assert L.mt_loudness_workspace_bytes(1, 4000, 8) == 0 and "hop 8" in last()
    assert L.mt_loudness_workspace_bytes(0, 4000, 800) == 0 and "B 0" in last()

    def tp(B=1, Ln=4000, half=40, audio=p, taps=p, tpeak=p, ws=p, ws_bytes=1 << 30):
        return L.mt_true_peak(audio, B, Ln, None, taps, half, None, tpeak, ws, ws_bytes, None)

    assert tp(B=0) != 0 and "true_peak: B 0" in last()
    assert tp(Ln=0) != 0 and "L 0" in last()
    assert tp(Ln=1 << 29) != 0 and "true_peak: B" in last()
    assert tp(half=0) != 0 and "half-length 0" in last()
    assert tp(half=1025) != 0 and "half-length 1025" in last()
    assert tp(audio=None) != 0 and "null argument" in last()
    assert tp(taps=None) != 0 and "null argument" in last()
    assert tp(tpeak=None) != 0 and "null argument" in last()
    assert tp(ws=None) != 0 and "workspace" in last()
    need = L.mt_true_peak_workspace_bytes(3, 1000)
    assert need == 4 * (4 * 513) + 3 * 2 * 4  # the table of the longest filter, then a partial per tile of 2048 outputs
    assert tp(B=3, Ln=1000, ws_bytes=need - 1) != 0 and "workspace too small" in last()
    assert L.mt_true_peak_workspace_bytes(1, 1 << 29) == 0 and "true_peak" in last()
    # the audio stage's own refusal that shapes this interface
    assert L.mt_audio_encode(p, 1, 16, None, p, p, 3, 1.0, 1, 0, p, None, None) != 0 and "normalisation mode 3" in last()


def test_audio_output_argument_refusals():
    from hifigan.output import AudioOutput, Loudness
    from matcha_hip import runtime as rt
    from matcha_hip._lib import HipPathError
    o = AudioOutput(16000, loudness=-16)
    assert o.loudness == -16.0 and o.true_peak == -1.0 and o.normalize is None and o.limit is True
    assert AudioOutput().loudness is None and AudioOutput(loudness=0.0, true_peak=0).true_peak == 0.0
    for kw in (dict(loudness=-16, normalize="peak"), dict(loudness=-16, normalize="rms"), dict(loudness=-70.0),
               dict(loudness=0.5), dict(loudness=float("nan")), dict(loudness=float("-inf")),
               dict(loudness=-16, true_peak=0.1), dict(loudness=-16, true_peak=float("nan")),
               dict(loudness=-16, true_peak=float("-inf")), dict(true_peak=1.0),
               dict(sample_rate=7350, loudness=-16), dict(normalize="lufs")):
        with pytest.raises(ValueError):
            AudioOutput(**kw)
    assert Loudness._fields == ("lufs", "true_peak_db", "lengths", "sample_rate")
    x = torch.zeros(2, 512)
    for fn in (lambda: o(x), lambda: o.measure(x), lambda: AudioOutput().measure(x),
               lambda: rt.loudness(x, None, 16000), lambda: rt.true_peak(x, None, None)):
        with pytest.raises(HipPathError):
            fn()
    with pytest.raises(ValueError):
        rt.loudness(x, None, 4000)
