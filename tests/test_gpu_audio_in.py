"""Recording input stage on the GPU (csrc/mt_audio_in.hip, hifigan/input.py): mt_audio_decode,
mt_log_mel_ragged, mel_spectrogram(lengths=) and hifigan.input.AudioInput against the CPU specification
matcha_hip/audio_in.py, the existing one-row featurizer (mt_log_mel, bit for bit) and the oracle.

  - decode: the bits of decode_ref for every encoding and 1..3 channels, zero past a row's length whatever the buffer
    holds there;
  - ragged log-mel: frames_ref, each row's frames torch.equal to mt_log_mel of gain * row[a:e] held alone (the wrong-end
    reflection and a read past e_b cannot hide: every sample outside [a_b, e_b) is NaN, and the lengths sit on both
    sides of every boundary), within the featurizer's 1e-4 of the oracle, `fill` past the frames out to Fcap;
  - a row's bits do not depend on the batch, the buffer's L or Fcap;
  - mt_resample into 22,050 Hz within the forward error bound of an fp32 FMA chain, |err| <= (Q + 1) 2^-24 A max|x|
    (Q taps per phase, A = max_p sum_q |P[p][q]|: derived from the taps, not measured), as the output-side test has it;
  - the whole stage against the composed specification, and its hand-over to MatchaTTS.align / edit.
"""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import make_matcha

from hifigan.meldataset import mel_basis, mel_spectrogram
from matcha_hip import audio_in as ai
from matcha_hip import audio_out as ao
from matcha_hip import join as jn
from matcha_hip import synthetic
from oracle import matcha_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
NP_DT = {"f32": np.float32, "pcm16": np.int16, "mulaw": np.uint8}


def _mel1(sig: torch.Tensor, **kw) -> torch.Tensor:
    """[n] -> [80, F] through the EXISTING kernel (mt_log_mel), the signal held alone"""
    return mel_spectrogram(sig.reshape(1, -1).to(DEV), 1024, 80, 22050, 256, 1024, 0, 8000, **kw)[0]


@functools.lru_cache(maxsize=None)
def _oracle_basis():
    return O.librosa_mel_basis(22050, 1024, 80, 0.0, 8000.0)


def _basis():
    return mel_basis(22050, 1024, 80, 0, 8000, torch.device(DEV, torch.cuda.current_device()))


# ---------------------------------------------------------------- 1. decode
@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("encoding", ["f32", "pcm16", "mulaw"])
def test_decode_bits_and_zero_past_the_length(encoding, channels):
    from matcha_hip import runtime as rt
    B, Lcap, lens = 4, 1024, [0, 1, 1000, 1024]
    rng = np.random.default_rng(17 + channels)
    n = B * Lcap * channels
    if encoding == "f32":
        raw = (rng.random(n, dtype=np.float32) * 2 - 1).astype(np.float32)
        raw[rng.integers(0, n, 40)] = np.array([np.nan, np.inf, -np.inf, 1e8] * 10, dtype=np.float32)
        junk = np.float32(np.nan)
    elif encoding == "pcm16":
        raw = rng.integers(-32768, 32768, n).astype(np.int16)
        junk = np.int16(-32768)    # 0x8000
    else:
        raw = rng.integers(0, 256, n).astype(np.uint8)
        junk = np.uint8(0x00)      # the most negative code
    raw = raw.reshape(B, Lcap * channels)
    for b, ln in enumerate(lens):
        raw[b, ln * channels:] = junk
    out = rt.decode_audio(torch.from_numpy(raw).to(DEV), torch.tensor(lens), encoding, channels).cpu().numpy()
    assert out.shape == (B, Lcap) and out.dtype == np.float32
    for b, ln in enumerate(lens):
        want = ai.decode_ref(raw[b, :ln * channels], encoding, channels)
        assert np.array_equal(out[b, :ln].view(np.uint32), want.view(np.uint32)), (b, ln)
        assert np.array_equal(out[b, ln:].view(np.uint32), np.zeros(Lcap - ln, np.uint32)), (b, ln)   # +0.0 exactly
    assert np.isfinite(out).all()
    # lengths=None: every row is Lcap frames long; a length outside [0, Lcap] is clamped
    full = rt.decode_audio(torch.from_numpy(raw).to(DEV), None, encoding, channels).cpu().numpy()
    over = rt.decode_audio(torch.from_numpy(raw).to(DEV), torch.tensor([-3, 5000, 1024, 1 << 30]), encoding,
                           channels).cpu().numpy()
    for b in range(B):
        want = ai.decode_ref(raw[b], encoding, channels)
        assert np.array_equal(full[b], want)
        assert np.array_equal(over[b], want if b else np.zeros(Lcap, np.float32))


# ---------------------------------------------------------------- 2. ragged log-mel
RAG_L = 8192
RAG_A = [0, 3, 255, 0, 3, 255, 3]
RAG_N = [0, 384, 385, 511, 512, 4113, RAG_L - 3]
RAG_GAIN = [0.5, 1.37, 2.0, 0.25, 1.0, 3.3, 0.77]


@functools.lru_cache(maxsize=None)
def _ragged_case():
    """-> (audio [7, 8192] host fp32, NaN outside [a_b, e_b); the rows' own signals)"""
    g = torch.Generator().manual_seed(2025)
    audio = torch.full((len(RAG_A), RAG_L), float("nan"))
    rows = []
    for b, (a, n) in enumerate(zip(RAG_A, RAG_N)):
        sig = (torch.rand(n, generator=g) * 2 - 1) * (0.1 + 0.1 * b)
        audio[b, a:a + n] = sig
        rows.append(sig)
    return audio, rows


@functools.lru_cache(maxsize=None)
def _ragged_refs(with_gain: bool):
    """per row with frames: (the existing kernel's mel of the row alone, the oracle's), computed once"""
    _, rows = _ragged_case()
    out = []
    for b, sig in enumerate(rows):
        if ai.frames_ref(sig.shape[0]) == 0:
            out.append(None)
            continue
        s = sig * torch.tensor(RAG_GAIN[b], dtype=torch.float32) if with_gain else sig
        out.append((_mel1(s).cpu(), O.mel_spectrogram(s[None], _oracle_basis())[0]))
    return out


@pytest.mark.parametrize("Fcap", [32, 37])
@pytest.mark.parametrize("with_gain", [False, True])
def test_ragged_log_mel_matches_the_one_row_kernel_bit_for_bit(with_gain, Fcap):
    from matcha_hip import runtime as rt
    audio, rows = _ragged_case()
    B = len(rows)
    assert ai.frames_ref(RAG_L) == 32
    start = torch.tensor(RAG_A, dtype=torch.int32)
    end = start + torch.tensor(RAG_N, dtype=torch.int32)
    gain = torch.tensor(RAG_GAIN, dtype=torch.float32).to(DEV) if with_gain else None
    fill = -11.5 if Fcap == 32 else 0.0
    mel, frames = rt.log_mel_ragged(audio.to(DEV), _basis(), start, end, gain, fill=fill, Fcap=Fcap)
    mel, frames = mel.cpu(), frames.cpu().tolist()
    assert mel.shape == (B, 80, Fcap)
    assert frames == [ai.frames_ref(n) for n in RAG_N] == [0, 0, 1, 1, 2, 16, 31]
    assert torch.isfinite(mel).all()
    refs = _ragged_refs(with_gain)
    for b in range(B):
        f = frames[b]
        assert torch.equal(mel[b, :, f:], torch.full((80, Fcap - f), fill)), b
        if f == 0:
            continue
        one, oracle = refs[b]
        assert one.shape == (80, f)
        assert torch.equal(mel[b, :, :f], one), (b, (mel[b, :, :f] - one).abs().max().item())
        err = (mel[b, :, :f] - oracle).abs().max().item()
        print(f"row {b} (a {RAG_A[b]}, n {RAG_N[b]}, gain {with_gain}): {f} frames, max|d| to the oracle {err:.2e}")
        assert err < 1e-4, (b, err)


def test_ragged_log_mel_statistics_nulls_and_clamped_tables():
    from matcha_hip import runtime as rt
    audio, rows = _ragged_case()
    # mel_mean / mel_std fused: the bits of the existing kernel's fused normalisation
    start = torch.tensor(RAG_A, dtype=torch.int32)
    end = start + torch.tensor(RAG_N, dtype=torch.int32)
    mel, frames = rt.log_mel_ragged(audio.to(DEV), _basis(), start, end, None, mel_mean=-5.536622, mel_std=2.116101)
    for b in (4, 5):
        f = int(frames[b])
        assert torch.equal(mel[b, :, :f], _mel1(rows[b], mel_mean=-5.536622, mel_std=2.116101))
    # start = end = None: every row whole, reflected at the buffer's ends like mt_log_mel itself
    g = torch.Generator().manual_seed(4)
    y = (torch.rand(2, 1500, generator=g) * 2 - 1).to(DEV)
    mel, frames = rt.log_mel_ragged(y, _basis())
    assert frames.tolist() == [5, 5]
    assert torch.equal(mel, mel_spectrogram(y, 1024, 80, 22050, 256, 1024, 0, 8000))
    # tables pointing outside the buffer are clamped: a = clamp(start, 0, L), e = clamp(end, a, L)
    st = torch.tensor([-7, 1000], dtype=torch.int32)
    en = torch.tensor([1 << 30, 400], dtype=torch.int32)
    mel2, frames2 = rt.log_mel_ragged(y, _basis(), st, en, fill=2.5)
    assert frames2.tolist() == [5, 0]
    assert torch.equal(mel2[0], mel[0]) and torch.equal(mel2[1], torch.full_like(mel2[1], 2.5))
    # a buffer too short for any frame: nothing but the counts
    mel3, frames3 = rt.log_mel_ragged(y[:, :384].contiguous(), _basis())
    assert mel3.shape == (2, 80, 0) and frames3.tolist() == [0, 0]


# ---------------------------------------------------------------- 3. batch invariance
def test_a_row_alone_in_another_buffer_has_the_same_bits():
    from matcha_hip import runtime as rt
    audio, rows = _ragged_case()
    start = torch.tensor(RAG_A, dtype=torch.int32)
    end = start + torch.tensor(RAG_N, dtype=torch.int32)
    gain = torch.tensor(RAG_GAIN, dtype=torch.float32).to(DEV)
    mel, frames = rt.log_mel_ragged(audio.to(DEV), _basis(), start, end, gain, fill=1.0)
    b, L1, a1, Fcap1 = 5, 5000, 17, 40
    alone = torch.full((1, L1), float("nan"))
    alone[0, a1:a1 + RAG_N[b]] = rows[b]
    mel1, frames1 = rt.log_mel_ragged(alone.to(DEV), _basis(), torch.tensor([a1]), torch.tensor([a1 + RAG_N[b]]),
                                      gain[b:b + 1], fill=1.0, Fcap=Fcap1)
    f = int(frames[b])
    assert f == 16 and frames1.tolist() == [f] and mel1.shape == (1, 80, Fcap1)
    assert torch.equal(mel1[0, :, :f], mel[b, :, :f])
    assert torch.equal(mel1[0, :, f:], torch.ones(80, Fcap1 - f, device=DEV))


def _recordings(seed: int, silent_row: int = 1):
    """Three 48 kHz stereo PCM16 recordings of about 0.05 s, 0.3 s and 0.5 s with a silent lead-in and tail, one of
    them all zeros -> (raw int16 [3, Lcap * 2] host, lens in frames). Past a row's length the buffer holds 0x8000."""
    rng = np.random.default_rng(seed)
    lens = [2400, 14400 + 37, 24000]
    Lcap = max(lens)
    raw = np.full((3, Lcap, 2), -32768, dtype=np.int16)
    for b, n in enumerate(lens):
        x = np.zeros((n, 2), dtype=np.float64)
        if b != silent_row:
            lead, tail = n // 10, n // 8
            t = np.arange(n - lead - tail) / 48000.0
            tone = 0.3 * np.sin(2 * np.pi * (180.0 + 90.0 * b) * t) + 0.1 * rng.standard_normal(t.shape[0])
            x[lead:n - tail, 0] = tone * (0.5 + 0.2 * b)
            x[lead:n - tail, 1] = tone * 0.3 + 0.02 * rng.standard_normal(t.shape[0])
        raw[b, :n] = np.rint(np.clip(x, -1, 1) * 32767).astype(np.int16)
    return raw.reshape(3, Lcap * 2), lens


def _stage():
    from hifigan.input import AudioInput
    return AudioInput(48000, "pcm16", channels=2, normalize="peak", trim_db=-40, trim_pad_ms=10)


def test_audio_input_rows_do_not_depend_on_the_batch():
    raw, lens = _recordings(5)
    inp = _stage()
    out = inp(torch.from_numpy(raw).to(DEV), torch.tensor(lens))
    for b, n in enumerate(lens):
        one = inp(torch.from_numpy(raw[b:b + 1, :n * 2].copy()).to(DEV))   # its own Lcap, lengths=None
        n22, ml = int(out.lengths[b]), int(out.mel_lengths[b])
        assert one.lengths.tolist() == [n22] and one.mel_lengths.tolist() == [ml]
        assert one.audio.shape[1] == ao.out_length(n, 147, 320) == n22
        assert torch.equal(one.audio[0], out.audio[b, :n22]) and not out.audio[b, n22:].any()
        assert torch.equal(one.gain[0], out.gain[b])
        assert torch.equal(one.start[0], out.start[b]) and torch.equal(one.end[0], out.end[b])
        assert one.mel.shape == (1, 80, ml) and torch.equal(one.mel[0], out.mel[b, :, :ml])


# ---------------------------------------------------------------- 4. resampling into 22,050 Hz
def _bound(plan, xmax):
    """(Q + 1) 2^-24 max_p sum_q |P[p][q]| max|x|: the forward error of an fp32 FMA chain of Q terms from 0"""
    P = np.abs(plan.taps_host.astype(np.float64))
    return (P.shape[1] + 1) * 2.0 ** -24 * P.sum(axis=1).max() * xmax


@pytest.mark.parametrize("src", [8000, 16000, 24000, 44100, 48000])
def test_resample_into_22050_against_fp64_reference(src):
    from matcha_hip import runtime as rt
    plan = rt.resample_plan(src, 22050, device=DEV)
    assert (plan.up, plan.down) == {8000: (441, 160), 16000: (441, 320), 24000: (147, 160), 44100: (1, 2),
                                    48000: (147, 320)}[src]
    B, L, lens = 4, 4096, [4096, 1, 0, 2049]
    x = torch.rand(B, L, generator=torch.Generator().manual_seed(src), dtype=torch.float64).mul_(2).sub_(1).float()
    y, ol = rt.resample(x.to(DEV), plan, torch.tensor(lens))
    y, ol = y.cpu().numpy(), ol.cpu().tolist()
    assert y.shape == (B, ao.out_length(L, plan.up, plan.down))
    assert ol == [ao.out_length(n, plan.up, plan.down) for n in lens]
    h32 = np.zeros(2 * plan.half + 1)
    P = plan.taps_host.astype(np.float64)                     # P[p][q] = h[q up + p]: the taps as the kernel holds them
    idx = np.arange(2 * plan.half + 1)
    h32[:] = P[idx % plan.up, idx // plan.up]
    worst = 0.0
    for b, n in enumerate(lens):
        assert not y[b, ol[b]:].any(), b
        if n == 0:
            continue
        xb = x[b, :n].numpy()
        ref = ao.resample_ref(xb, plan.up, plan.down, h32, plan.half)
        err, bound = np.abs(y[b, :ol[b]] - ref).max(), _bound(plan, np.abs(xb).max())
        worst = max(worst, err / bound)
        assert err <= bound, (b, err, bound)
    print(f"{src}->22050: max err / bound {worst:.3f}")


# ---------------------------------------------------------------- 5. the stage against the composed specification
def test_audio_input_matches_the_composed_specification():
    from matcha_hip import runtime as rt
    raw, lens = _recordings(9)
    inp = _stage()
    out = inp(torch.from_numpy(raw).to(DEV), torch.tensor(lens))
    B, Lcap = 3, max(lens)
    # decode_ref of every row, through the existing resampler: bit for bit
    x = np.zeros((B, Lcap), dtype=np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = ai.decode_ref(raw[b, :n * 2], "pcm16", 2)
    plan = rt.resample_plan(48000, 22050, device=DEV)
    want_audio, want_lens = rt.resample(torch.from_numpy(x).to(DEV), plan, torch.tensor(lens))
    assert out.audio.dtype == torch.float32 and torch.equal(out.audio, want_audio)
    assert out.lengths.dtype == torch.int32 and torch.equal(out.lengths, want_lens)
    assert out.mel_lengths.dtype == torch.int64 and out.start.dtype == out.end.dtype == torch.int32
    audio = out.audio.cpu().numpy()
    thr, pad = float(np.float32(10.0 ** (-40 / 20.0))), 220
    assert (inp.thr, inp.pad) == (thr, pad)
    assert out.mel.shape == (B, 80, int(out.mel_lengths.max()))
    for b in range(B):
        n22 = int(out.lengths[b])
        a, e = jn.edges_ref(audio[b], n22, thr, pad)
        assert (int(out.start[b]), int(out.end[b])) == (a, e), b
        g = ao.gain_ref(np.abs(audio[b, :n22]).max(), None, "peak", 0.95)
        assert np.float32(out.gain[b].item()) == g, (b, out.gain[b].item(), g)
        f = ai.frames_ref(e - a)
        assert int(out.mel_lengths[b]) == f
        assert torch.equal(out.mel[b, :, f:], torch.zeros(80, out.mel.shape[2] - f, device=DEV))
        if b == 1:   # the silent row
            assert (a, e, f) == (0, 0, 0) and g == 1.0
            continue
        assert a < e <= n22 and f > 0
        if b == 2:
            assert 500 < a and e < n22 - 500        # the lead-in (0.05 s) and the tail were cut, less the 10 ms pad
        sig = torch.from_numpy(audio[b, a:e]) * torch.tensor(float(g), dtype=torch.float32)
        assert torch.equal(out.mel[b, :, :f], _mel1(sig)), b
        peak = float(np.abs(sig.numpy()).max())
        assert abs(peak - 0.95) < 1e-6              # the loudest sample lies inside the trimmed range
    # at 22,050 Hz mono f32 without level or trim the stage is decode + featurizer
    from hifigan.input import AudioInput
    y = torch.from_numpy(audio[2:3, :3000].copy())
    o2 = AudioInput(22050, mel_mean=-5.5, mel_std=2.1, fill=-1.0)(y.to(DEV), torch.tensor([2000]))
    assert o2.lengths.tolist() == [2000] and o2.mel_lengths.tolist() == [7] and o2.gain.tolist() == [1.0]
    assert (o2.start.tolist(), o2.end.tolist()) == ([0], [2000])
    assert torch.equal(o2.audio[0, :2000], y[0, :2000].to(DEV)) and not o2.audio[0, 2000:].any()
    assert torch.equal(o2.mel[0], _mel1(y[0, :2000], mel_mean=-5.5, mel_std=2.1))


# ---------------------------------------------------------------- 6. mel_spectrogram(lengths=)
def test_mel_spectrogram_with_lengths_equals_the_per_row_calls():
    from matcha_hip._lib import lib, stream_handle
    g = torch.Generator().manual_seed(6)
    L, lens = 5000, [5000, 385, 2500, 200]
    y = (torch.rand(4, L, generator=g) * 2 - 1) * 0.7
    padded = y.clone()
    for b, n in enumerate(lens):
        padded[b, n:] = float("nan")
    args = (1024, 80, 22050, 256, 1024, 0, 8000)
    for kw in (dict(), dict(mel_mean=-5.536622, mel_std=2.116101)):
        mel = mel_spectrogram(padded.to(DEV), *args, lengths=torch.tensor(lens), **kw)
        assert mel.shape == (4, 80, ai.frames_ref(L))
        for b, n in enumerate(lens):
            f = ai.frames_ref(n)
            assert not mel[b, :, f:].any()
            if f:
                assert torch.equal(mel[b, :, :f], mel_spectrogram(y[b, :n].to(DEV), *args, **kw)), (b, kw)
    # without lengths nothing changed: the bits of a direct call of mt_log_mel on the same buffer
    yd = y.to(DEV)
    direct = torch.empty(4, 80, ai.frames_ref(L), device=DEV)
    assert lib().mt_log_mel(yd.data_ptr(), 4, L, _basis().data_ptr(), 0.0, 1.0, direct.data_ptr(),
                            stream_handle(yd.device)) == 0
    assert torch.equal(mel_spectrogram(yd, *args), direct)
    # ... and its rows are reflected at L, which is what lengths= is for
    assert not torch.equal(mel_spectrogram(yd, *args)[2, :, :9], mel_spectrogram(y[2, :2500].to(DEV), *args))


# ---------------------------------------------------------------- 7. hand-over to align and edit
def test_the_stage_feeds_align_and_edit():
    from hifigan.input import AudioInput
    m = make_matcha(1, "fp32")
    sd = {k: torch.from_numpy(v) for k, v in synthetic.make_state_dict(
        [(k, tuple(v.shape)) for k, v in m.state_dict().items()], 1, force_log_duration=math.log(1.5)).items()}
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    x, xl = synthetic.synthetic_text(2, seed=3, lo=9, hi=12)
    x, xl = torch.from_numpy(x).to(DEV), torch.from_numpy(xl).to(DEV)
    lo = xl.tolist()
    # two 16 kHz mono mu-law "recordings" of 0.45 s and 0.3 s
    rng = np.random.default_rng(8)
    lens = [7200, 4800]
    pcm = np.rint(np.clip(0.2 * rng.standard_normal((2, 7200)), -1, 1) * 32767).astype(np.int16)
    raw = ao.mulaw_ref(pcm)
    out = AudioInput(16000, "mulaw", normalize="peak")(torch.from_numpy(raw).to(DEV), torch.tensor(lens))
    ml = out.mel_lengths.tolist()
    assert ml == [ai.frames_ref(ao.out_length(n, 441, 320)) for n in lens] and min(ml) > max(lo)
    d = m.align(x, xl, out.mel, out.mel_lengths)
    assert d.shape == x.shape and d.sum(1).tolist() == ml
    for b in range(2):
        assert bool((d[b, :lo[b]] >= 1).all()) and not d[b, lo[b]:].any()
    # replace tokens [3, 5) by three others: every frame outside the span is the recording's
    x_new = torch.zeros(2, x.shape[1] + 1, dtype=x.dtype, device=DEV)
    spans = []
    for b in range(2):
        x_new[b, :3] = x[b, :3]
        x_new[b, 3:6] = torch.tensor([31, 32, 33], device=DEV) + b
        x_new[b, 6:lo[b] + 1] = x[b, 5:lo[b]]
        spans.append((3, 5, 6))
    mel, yl, keep = m.edit(x, xl, out.mel, out.mel_lengths, x_new, xl + 1, spans, 2, durations_old=d, seeds=[1, 2])
    assert torch.isfinite(mel).all() and keep.dtype == torch.bool and keep.shape == (2, mel.shape[-1])
    for b in range(2):
        f_a, f_b = int(d[b, :3].sum()), int(d[b, :5].sum())
        tail = ml[b] - f_b
        y_new = int(yl[b])
        assert keep[b, :f_a].all() and keep[b, y_new - tail:y_new].all() and not keep[b, f_a:y_new - tail].any()
        # normalize, the solve's exact x1 and denormalize are three fp32 roundings on values below 16 (ulp 9.5e-7)
        pre = (mel[b, :, :f_a] - out.mel[b, :, :f_a]).abs().max().item()
        post = (mel[b, :, y_new - tail:y_new] - out.mel[b, :, f_b:ml[b]]).abs().max().item()
        print(f"edit row {b}: {f_a} + {tail} kept frames, max|d| {pre:.2e} / {post:.2e}")
        assert pre <= 1e-5 and post <= 1e-5, (b, pre, post)
