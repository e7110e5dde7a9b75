"""Streaming waveform delivery (hifigan/stream.py, csrc/mt_stream.hip, mt_resample_range): the
concatenated chunks of a row are, bit for bit, that row of the one-shot path, for the vocoder alone, with the
denoiser, and through the output stage; a stream with no halo is not (so the equalities mean something); step c
reads no mel frame at or past e_c + reach; mt_resample_range's slices are mt_resample's bits and read nothing past
the last sample their chains touch.
"""
import pytest
import torch

from conftest import make_generator

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, T = 6, 64
LENGTHS = [61, 32, 17, 1, 0, 45]
STRENGTH = 0.00025


def _gen(precision, seed=8):
    from matcha_hip import synthetic
    g = make_generator(precision)
    sd = synthetic.make_state_dict([(k, tuple(v.shape)) for k, v in g.state_dict().items()], seed)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    g = g.to(DEV).eval()
    g.remove_weight_norm()
    return g


def _mel(b, t, seed=9):
    return torch.randn(b, 80, t, generator=torch.Generator().manual_seed(seed)) * 2.1 - 5.5


@pytest.fixture(scope="module")
def ctx():
    """the bf16 generator, its denoiser, the mel and the one-shot results every test compares against"""
    from hifigan.denoiser import Denoiser
    g = _gen("bf16")
    den = Denoiser(g, mode="zeros")
    mel = _mel(B, T).to(DEV)
    lens = torch.tensor(LENGTHS, device=DEV)
    wav = g(mel, lens)
    clean = den(wav.squeeze(1), STRENGTH, lens)
    torch.cuda.synchronize()
    return dict(g=g, den=den, mel=mel, lens=lens, wav=wav[:, 0].clone(), clean=clean.clone())


def _stitch(chunks, n_rows):
    """-> (rows: the concatenated valid samples of each row, number of chunks); checks offset / lengths / done"""
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


@pytest.mark.parametrize("chunk,first", [(16, None), (5, None), (32, 8)])
def test_vocoder_stream_equals_one_shot(ctx, chunk, first):
    from hifigan.stream import WaveStreamer
    s = WaveStreamer(ctx["g"], chunk_frames=chunk, first_chunk_frames=first)
    assert ctx["g"].receptive_field() == 13
    rows, n = _stitch(s(ctx["mel"], ctx["lens"]), B)
    assert n == len(s.schedule(LENGTHS)) and n > 1
    out = torch.zeros_like(ctx["wav"])
    for b, r in enumerate(rows):
        assert r.dtype == torch.float32 and r.numel() == 256 * LENGTHS[b], (b, r.numel())
        out[b, :r.numel()] = r
    assert torch.equal(out, ctx["wav"]), (out - ctx["wav"]).abs().amax(dim=1)
    for b in range(B):
        assert torch.count_nonzero(out[b, 256 * LENGTHS[b]:]) == 0


def test_vocoder_stream_without_halo_differs(ctx):
    """negative control: the same stream with the halo forced to 0 is NOT the one-shot result on the 61-frame row"""
    from hifigan.stream import WaveStreamer
    s = WaveStreamer(ctx["g"], chunk_frames=16, _halo=0)
    rows, _ = _stitch(s(ctx["mel"], ctx["lens"]), B)
    assert rows[0].numel() == 256 * 61
    assert not torch.equal(rows[0], ctx["wav"][0, :256 * 61])


@pytest.mark.parametrize("chunk", [16, 5])
def test_vocoder_denoiser_stream_equals_one_shot(ctx, chunk):
    """chunk 5: odd window ends; the windows must still start on even frames (the kernel's frame pairs)"""
    from hifigan.stream import WaveStreamer
    s = WaveStreamer(ctx["g"], ctx["den"], chunk_frames=chunk, strength=STRENGTH)
    rows, _ = _stitch(s(ctx["mel"], ctx["lens"]), B)
    for b, r in enumerate(rows):
        n = 256 * LENGTHS[b]
        assert r.numel() == n
        assert torch.equal(r, ctx["clean"][b, :n]), (b, (r - ctx["clean"][b, :n]).abs().max())


@pytest.mark.parametrize("rate,enc", [(22050, "f32"), (16000, "pcm16"), (8000, "mulaw"), (48000, "f32")])
def test_whole_chain_stream_equals_one_shot(ctx, rate, enc):
    from hifigan.output import AudioOutput
    from hifigan.stream import WaveStreamer
    o = AudioOutput(rate, encoding=enc)
    ref = o(ctx["clean"], ctx["lens"])
    s = WaveStreamer(ctx["g"], ctx["den"], o, chunk_frames=16, first_chunk_frames=8, strength=STRENGTH)
    rows, _ = _stitch(s(ctx["mel"], ctx["lens"]), B)
    ref_lens = ref.lengths.tolist()
    for b, r in enumerate(rows):
        assert r.dtype == ref.audio.dtype and r.numel() == ref_lens[b], (b, r.numel(), ref_lens[b])
        assert torch.equal(r, ref.audio[b, :ref_lens[b]]), b


def test_level_normalisation_is_refused(ctx):
    from hifigan.output import AudioOutput
    from hifigan.stream import WaveStreamer
    for mode in ("peak", "rms"):
        with pytest.raises(ValueError, match="whole utterance"):
            WaveStreamer(ctx["g"], ctx["den"], AudioOutput(16000, normalize=mode, encoding="pcm16"))


def test_stream_reads_no_frame_past_its_reach(ctx):
    """the mel is NaN beyond what each step may read and is filled in, frame by frame, before each step: the result
    is still the one-shot result of the true mel"""
    from hifigan.stream import WaveStreamer
    first, chunk = 8, 16
    s = WaveStreamer(ctx["g"], ctx["den"], chunk_frames=chunk, first_chunk_frames=first, strength=STRENGTH)
    reach = ctx["g"].receptive_field()
    true = ctx["mel"]
    mel = true.clone()
    mel[..., reach + first:] = float("nan")
    ends = s.schedule(LENGTHS)
    it = s(mel, ctx["lens"])
    chunks = []
    for e in ends:
        mel[..., :e + reach] = true[..., :e + reach]
        ch = next(it)
        assert torch.isfinite(ch.audio).all()
        chunks.append(ch)
    with pytest.raises(StopIteration):
        next(it)
    rows, _ = _stitch(chunks, B)
    for b, r in enumerate(rows):
        n = 256 * LENGTHS[b]
        assert torch.equal(r, ctx["clean"][b, :n]), b


def test_resample_range_slices_are_resample_bits():
    from matcha_hip import runtime as rt
    from matcha_hip import stream_plan as sp
    Bn, L = 3, 5000
    lens = torch.tensor([5000, 1234, 0], dtype=torch.int32, device=DEV)
    audio = (torch.randn(Bn, L, generator=torch.Generator().manual_seed(2)) * 0.3).to(DEV)
    plan = rt.resample_plan(22050, 16000, device=DEV)
    assert (plan.up, plan.down) == (320, 441)
    full, full_lens = rt.resample(audio, plan, lens)
    n_out = full_lens.tolist()
    end = full.shape[1]
    parts, counts = [], []
    for lo, hi in ((0, 700), (700, 701), (701, end)):
        a = audio.clone()
        last = sp.resample_last_read(hi, plan.up, plan.down, plan.half)
        a[:, last + 1:] = float("nan")  # nothing past the last sample the range's chains touch is read
        out, cnt = rt.resample_range(a, plan, lens, 1, lo, hi - lo)
        assert out.shape == (Bn, hi - lo)
        assert cnt.tolist() == [min(max(n - lo, 0), hi - lo) for n in n_out]
        parts.append(out)
        counts.append(cnt)
    got = torch.cat(parts, dim=1)
    assert torch.isfinite(got).all()
    assert torch.equal(got, full)
    assert torch.equal(sum(counts), full_lens)
    with pytest.raises(Exception, match="resample_range"):
        rt.resample_range(audio, plan, lens, 1, 0, 0)


def test_window_gather_scatter_clamp_bad_tables():
    """a table entry outside its buffer reads zeros / writes nothing"""
    from matcha_hip import runtime as rt
    src = torch.arange(2 * 3 * 10, dtype=torch.float32, device=DEV).reshape(2, 3, 10)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)  # noqa: E731
    rows = rt.window_gather(src, i32([1, 0, 5, 0, 1]), i32([2, 7, 0, -1, 0]), i32([4, 9, 3, 2, -3]), 6)
    want = torch.zeros(5, 3, 6, device=DEV)
    want[0, :, :4] = src[1, :, 2:6]
    want[1, :, :3] = src[0, :, 7:10]
    assert torch.equal(rows, want)
    dst = torch.full((2, 8), -1.0, device=DEV)
    win = torch.arange(4 * 6, dtype=torch.float32, device=DEV).reshape(4, 6)
    rt.window_scatter(win, i32([1, 0, 7, 0]), i32([1, 4, 0, -2]), i32([2, 6, 0, 0]), i32([3, 5, 2, 2]), dst)
    want = torch.full((2, 8), -1.0, device=DEV)
    want[1, 2:5] = win[0, 1:4]
    want[0, 6:8] = win[1, 4:6]
    assert torch.equal(dst, want)


def test_fp32_engine_stream():
    """fp32 (parity mode): the same plan with one vocoder call per window. The bar the fp32 ragged test sets for rows
    against one-utterance calls is 1e-5 (the generic kernel may pick another tile shape for another batch); measured
    on the MI355X the stitched rows are bit-identical to the one-shot ragged batch (max |d| 0), so that is asserted."""
    from hifigan.stream import WaveStreamer
    g = _gen("fp32")
    lens = [40, 9]
    mel = _mel(2, 48, seed=5).to(DEV)
    ref = g(mel, torch.tensor(lens, device=DEV))[:, 0]
    rows, _ = _stitch(WaveStreamer(g, chunk_frames=16)(mel, lens), 2)
    for b, r in enumerate(rows):
        n = 256 * lens[b]
        assert r.numel() == n
        err = float((r - ref[b, :n]).abs().max())
        print(f"fp32 row {b}: max |d| {err:.3e}")
        assert err < 1e-5, (b, err)
        assert torch.equal(r, ref[b, :n]), (b, err)
