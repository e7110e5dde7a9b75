"""Long-form join on the GPU (csrc/mt_join.hip, hifigan/longform.py): mt_audio_edges, mt_join_plan and
mt_join against the CPU specification matcha_hip/join.py, and LongForm end to end. Every comparison is exact:
integers equal, floats equal by value (np.array_equal / torch.equal).

  - edges: row ends and loud samples round the kernel's tile, NaN and loud values in the padding;
  - plan: segment counts round a wave and the scan chunk, documents of 0, 1 and many segments, empty segments, edges
    outside the row, gaps of both signs, the `bad` flag;
  - join: lengths round the tile and under two fades, overlaps by one fade and by far more, NaN round every kept
    range, a longer output row; the overlap is the two-rounding sum, on data where an FMA would differ;
  - a document alone equals its row of the batch, a permutation of the documents permutes the rows;
  - LongForm equals join_ref + AudioOutput.finish on its own segments, bit for bit.

Batching: measured on the MI355X, on the synthetic fp32 weights of this test `LongForm.segments` is NOT bit-equal
between max_batch = 1 and 32: a sentence's mel depends on the frame count its batch is padded to, as in the reference
(DESIGN.md §5); the stages after it are bit-stable. test_longform_does_not_depend_on_the_batching therefore compares
lengths and the sentence table, which are equal, and compares bytes only in a run where it first finds the rows
bit-equal. No tolerance stands in for that.
"""
import math

import numpy as np
import pytest
import torch

from conftest import make_generator, make_matcha

from matcha_hip import join as jn

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _i32(a):
    return torch.tensor(np.asarray(a, dtype=np.int64).tolist(), dtype=torch.int32, device=DEV)


def _np(t):
    return t.cpu().numpy()


# ---- edges ----------------------------------------------------------------------------------------------------

def _edge_rows():
    """-> (audio [S][L] fp32, lens [S]): four plantings for each of the six lengths; the padding past n is NaN on
    even rows and loud on odd ones"""
    from matcha_hip import runtime as rt
    T = rt.EDGES_TILE
    thr = np.float32(0.01)
    lens, rows = [], []
    L = 2 * T + 8
    rng = np.random.default_rng(3)
    for n in (0, 1, T - 1, T, T + 1, 2 * T + 3):
        for plant in ("first", "last", "boundary", "threshold"):
            x = (rng.standard_normal(L) * 1e-4).astype(np.float32)   # far under thr
            if n > 0:
                if plant == "first":
                    x[0] = 0.5
                elif plant == "last":
                    x[n - 1] = -0.5
                elif plant == "boundary":       # both sides of every tile boundary inside the row
                    for k in (T - 1, T, 2 * T - 1, 2 * T):
                        if k < n:
                            x[k] = 0.25
                    x[min(7, n - 1)] = np.nan   # a NaN inside the row is not loud
                else:                           # exactly thr is loud, the next fp32 under it is not
                    x[n // 2] = -thr
                    x[n - 1] = np.nextafter(thr, np.float32(0))
                    x[0] = np.nextafter(thr, np.float32(0))
            x[n:] = np.nan if len(rows) % 2 == 0 else 1.0
            rows.append(x)
            lens.append(n)
    return np.stack(rows), np.asarray(lens), float(thr)


@pytest.mark.parametrize("pad", [0, 5, 3 * 4096])
def test_edges_match_the_specification(pad):
    from matcha_hip import runtime as rt
    audio, lens, thr = _edge_rows()
    start, end = rt.audio_edges(torch.from_numpy(audio).to(DEV), _i32(lens), thr, pad)
    want = [jn.edges_ref(audio[s], int(lens[s]), thr, pad) for s in range(len(lens))]
    assert start.dtype == end.dtype == torch.int32
    assert np.array_equal(_np(start), [w[0] for w in want]) and np.array_equal(_np(end), [w[1] for w in want])
    assert any(w != (0, 0) for w in want) and any(w == (0, 0) for w in want)


def test_edges_lengths_clamp_and_none():
    from matcha_hip import runtime as rt
    audio, lens, thr = _edge_rows()
    S, L = audio.shape
    # lengths past L and negative are clamped into [0, L]; None means L
    wild = lens.copy()
    wild[0], wild[1], wild[-1] = -5, L + 100, 2 ** 31 - 1
    start, end = rt.audio_edges(torch.from_numpy(audio).to(DEV), _i32(wild), thr, 2)
    want = [jn.edges_ref(audio[s], min(max(int(wild[s]), 0), L), thr, 2) for s in range(S)]
    assert np.array_equal(_np(start), [w[0] for w in want]) and np.array_equal(_np(end), [w[1] for w in want])
    start, end = rt.audio_edges(torch.from_numpy(audio).to(DEV), None, thr, 2)
    want = [jn.edges_ref(audio[s], L, thr, 2) for s in range(S)]
    assert np.array_equal(_np(start), [w[0] for w in want]) and np.array_equal(_np(end), [w[1] for w in want])


# ---- plan -----------------------------------------------------------------------------------------------------

def _plan_case(S, seed):
    rng = np.random.default_rng(seed)
    L = 400
    # documents of 0, 1 and many segments: an empty one first, one segment, a long one, an empty one, small ones
    sizes = [0, 1] if S > 1 else [0]
    rest = S - sum(sizes)
    big = rest if S < 8 else int(rest * 0.6)
    sizes += [big, 0]
    rest -= big
    while rest > 0:
        k = int(min(rest, rng.integers(1, 6)))
        sizes.append(k)
        rest -= k
    sizes.append(0)
    doc_first = np.concatenate([[0], np.cumsum(sizes)])
    assert doc_first[-1] == S
    start = rng.integers(-20, L, S)                   # some before the row
    end = start + rng.integers(-30, 300, S)           # some empty, some past the row
    end[rng.integers(0, S, max(S // 6, 1))] = 0       # more empty segments
    gap = rng.integers(-2 * L, L, S)
    gap[rng.integers(0, S, max(S // 4, 1))] = rng.integers(-8, 9, max(S // 4, 1))
    return doc_first, start, end, gap, L


@pytest.mark.parametrize("S", [1, 63, 64, 65, 1025])
def test_plan_matches_the_specification(S):
    from matcha_hip import runtime as rt
    doc_first, start, end, gap, L = _plan_case(S, 100 + S)
    for head, tail in ((0, 0), (7, 11)):
        dst, doc_len, bad = rt.join_plan(_i32(doc_first), _i32(start), _i32(end), _i32(gap), head, tail, L)
        w_dst, w_len, w_bad = jn.plan_ref(doc_first, start, end, gap, head, tail, L)
        assert np.array_equal(_np(dst), w_dst) and np.array_equal(_np(doc_len), w_len)
        assert int(bad.item()) == w_bad == 0
    if S > 8:
        assert (np.diff(doc_first) > rt.JOIN_PLAN_CHUNK).any() == (S == 1025)   # only then a scan carries over


def test_plan_sets_bad_and_clamps():
    from matcha_hip import runtime as rt
    doc_first, start, end, gap, L = _plan_case(1025, 7)
    w_len = jn.plan_ref(doc_first, start, end, gap, 3, 4, L)[1]
    Lcap = int(w_len.max()) // 2
    dst, doc_len, bad = rt.join_plan(_i32(doc_first), _i32(start), _i32(end), _i32(gap), 3, 4, L, Lcap=Lcap)
    w_dst, w_len, w_bad = jn.plan_ref(doc_first, start, end, gap, 3, 4, L, Lcap=Lcap)
    assert w_bad == 1 and int(bad.item()) == 1
    assert np.array_equal(_np(dst), w_dst) and np.array_equal(_np(doc_len), w_len) and w_len.max() == Lcap
    # 64-bit inside: gaps that sum far past 2^31
    gap[:] = 2 ** 31 - 1
    dst, doc_len, bad = rt.join_plan(_i32(doc_first), _i32(start), _i32(end), _i32(gap), 3, 4, L)
    w_dst, w_len, w_bad = jn.plan_ref(doc_first, start, end, gap, 3, 4, L)
    assert w_bad == 1 and int(bad.item()) == 1 and w_len.max() == 1 << 30
    assert np.array_equal(_np(dst), w_dst) and np.array_equal(_np(doc_len), w_len)
    seg = torch.zeros(1025, L, device=DEV)
    with pytest.raises(ValueError, match="longer than"):
        rt.join(seg, _i32(start), _i32(end), _i32(doc_first), dst, doc_len, 0, bad=bad)


# ---- join -----------------------------------------------------------------------------------------------------

FADE = 48


@pytest.fixture(scope="module")
def joined():
    """four documents (many segments, one, none, several), their tables, the specification's result (computed once)
    and the kernels' result"""
    from matcha_hip import runtime as rt
    J = rt.JOIN_TILE
    rng = np.random.default_rng(11)
    lens = [J + 1, 0, 1, 2, 3, 2 * FADE - 1, 2 * FADE, 2 * FADE + 1, J - 1, J, 2 * J + 5, 5, 700,   # document 0
            J + 300,                                                                            # document 1
            300, 2 * J, 37, 4 * FADE, 900]                                                      # document 3
    doc_first = np.array([0, 13, 14, 14, 19])
    S = len(lens)
    a = rng.integers(0, 8, S)
    L = 2 * J + 5 + 8 + 3
    seg = np.full((S, L), np.nan, np.float32)            # NaN before a_s and from e_s on
    for s in range(S):
        seg[s, a[s]:a[s] + lens[s]] = rng.standard_normal(lens[s]).astype(np.float32)
    start, end = a, a + np.asarray(lens)
    gap = np.array([-FADE, 0, -1, -1, -FADE, -FADE, -10 * L, 17, -FADE, -10 * L, -FADE, -2, 0,
                    0,
                    -FADE, -10 * L, -FADE, 60, 0])
    head, tail = 5, 9
    w_dst, w_len, w_bad = jn.plan_ref(doc_first, start, end, gap, head, tail, L)
    Ld = int(w_len.max()) + J + 3                        # longer than every document: the rest is zero
    want = jn.join_ref(seg, start, end, doc_first, w_dst, w_len, FADE, Ld=Ld)
    t = dict(seg=torch.from_numpy(seg).to(DEV), start=_i32(start), end=_i32(end), doc_first=_i32(doc_first),
             gap=_i32(gap))
    dst, doc_len, bad = rt.join_plan(t["doc_first"], t["start"], t["end"], t["gap"], head, tail, L)
    out = rt.join(t["seg"], t["start"], t["end"], t["doc_first"], dst, doc_len, FADE, bad=bad, Ld=Ld)
    torch.cuda.synchronize()
    return dict(t, seg_np=seg, lens=np.asarray(lens), a=a, gap_np=gap, doc_first_np=doc_first, head=head, tail=tail,
                L=L, Ld=Ld, w_dst=w_dst, w_len=w_len, want=want, dst=dst, doc_len=doc_len, out=out)


def test_join_matches_the_specification(joined):
    j = joined
    assert np.array_equal(_np(j["dst"]), j["w_dst"]) and np.array_equal(_np(j["doc_len"]), j["w_len"])
    out = _np(j["out"])
    assert out.shape == j["want"].shape == (4, j["Ld"]) and out.dtype == np.float32
    assert np.isfinite(out).all()                        # no NaN from outside [a_s, e_s) came in
    assert np.array_equal(out, j["want"])
    for d in range(4):
        assert not out[d, j["w_len"][d]:].any()          # zero from doc_len on
    assert j["w_len"][2] == j["head"] + j["tail"] and not out[2].any()   # the empty document
    assert not out[:, :j["head"]].any()


def test_join_default_length_is_the_longest_document(joined):
    from matcha_hip import runtime as rt
    j = joined
    out = rt.join(j["seg"], j["start"], j["end"], j["doc_first"], j["dst"], j["doc_len"], FADE)
    n = int(j["w_len"].max())
    assert out.shape == (4, n) and torch.equal(out, j["out"][:, :n])
    # fade = 0: plain placement and sums, no table
    out0 = rt.join(j["seg"], j["start"], j["end"], j["doc_first"], j["dst"], j["doc_len"], 0)
    want0 = jn.join_ref(j["seg_np"], _np(j["start"]), _np(j["end"]), j["doc_first_np"], j["w_dst"], j["w_len"], 0)
    assert np.array_equal(_np(out0), want0)


def test_overlap_is_the_two_rounding_sum_not_an_fma(joined):
    """Where two segments cover a sample the result is fl(fl(w1 x1) + fl(w2 x2)). The CPU part shows that this data
    tells the two apart: for a sample with |a| within [2^-20, 16] of |p| the fp64 sum a + w2 x2 is exact (a has 24
    bits, the product 48, together under 53), so its one rounding to fp32 is what an FMA would give."""
    j = joined
    table = jn.ramp(FADE)
    out = _np(j["out"])
    differ = checked = 0
    for d in range(4):
        lo, hi = j["doc_first_np"][d], j["doc_first_np"][d + 1]
        for s in range(lo, hi - 1):
            n1, n2 = int(j["lens"][s]), int(j["lens"][s + 1])
            ov = int(j["w_dst"][s] + n1 - j["w_dst"][s + 1])
            if ov <= 0:
                continue
            w1 = jn.weights_ref(n1, FADE, table)[n1 - ov:]
            w2 = jn.weights_ref(n2, FADE, table)[:ov]
            x1 = j["seg_np"][s, j["a"][s] + n1 - ov:j["a"][s] + n1]
            x2 = j["seg_np"][s + 1, j["a"][s + 1]:j["a"][s + 1] + ov]
            acc = (w1 * x1).astype(np.float32)           # 0 + fl(w1 x1) is exact
            two = acc + (w2 * x2).astype(np.float32)
            p = w2.astype(np.float64) * x2.astype(np.float64)
            fma = (acc.astype(np.float64) + p).astype(np.float32)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.abs(acc.astype(np.float64)) / np.abs(p)
            ok = (r >= 2.0 ** -20) & (r <= 16.0)
            # a third segment may cover part of this span only if the plan were wrong: join_ref is the full check
            i0 = int(j["w_dst"][s + 1])
            got = out[d, i0:i0 + ov]
            single = np.ones(ov, bool)
            if s + 2 < hi:
                single[max(int(j["w_dst"][s + 2]) - i0, 0):] = False
            if s > lo:
                single[:max(int(j["w_dst"][s - 1] + j["lens"][s - 1]) - i0, 0)] = False
            assert np.array_equal(got[single], two[single])
            differ += int(((fma != two) & ok & single).sum())
            checked += int((ok & single).sum())
    print(f"overlap samples checked {checked}, of which an FMA would differ on {differ}")
    assert checked >= 4 * FADE and differ >= 1


def _chain(seg, start, end, gap, doc_first, head, tail, Ld):
    from matcha_hip import runtime as rt
    dst, doc_len, bad = rt.join_plan(doc_first, start, end, gap, head, tail, seg.shape[1])
    return rt.join(seg, start, end, doc_first, dst, doc_len, FADE, bad=bad, Ld=Ld), doc_len


def test_a_document_alone_equals_its_row_of_the_batch(joined):
    j = joined
    for d in range(4):
        lo, hi = int(j["doc_first_np"][d]), int(j["doc_first_np"][d + 1])
        if lo == hi:
            continue   # no segment to pass; its row is silence (test_join_matches_the_specification)
        out, doc_len = _chain(j["seg"][lo:hi].contiguous(), j["start"][lo:hi].contiguous(),
                              j["end"][lo:hi].contiguous(), j["gap"][lo:hi].contiguous(), _i32([0, hi - lo]),
                              j["head"], j["tail"], j["Ld"])
        assert torch.equal(out[0], j["out"][d]) and int(doc_len[0]) == int(j["w_len"][d])


def test_permuting_documents_permutes_rows(joined):
    j = joined
    perm = [3, 2, 0, 1]
    rows = np.concatenate([np.arange(j["doc_first_np"][d], j["doc_first_np"][d + 1]) for d in perm])
    sizes = [int(j["doc_first_np"][d + 1] - j["doc_first_np"][d]) for d in perm]
    idx = torch.from_numpy(rows).to(DEV)
    out, doc_len = _chain(j["seg"][idx].contiguous(), j["start"][idx].contiguous(), j["end"][idx].contiguous(),
                          j["gap"][idx].contiguous(), _i32(np.concatenate([[0], np.cumsum(sizes)])), j["head"],
                          j["tail"], j["Ld"])
    assert torch.equal(out, j["out"][perm]) and np.array_equal(_np(doc_len), j["w_len"][perm])


# ---- end to end -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tts():
    """the smallest models of the conftest factories on synthetic weights (1.5 -> 2 frames per token), two documents
    of three short sentences"""
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


def _longform(tts, output, under_peak_db=3.0, **kw):
    """-> (LongForm, its segments). under_peak_db: trim_db is set that far under the loudest sample of these
    sentences, because synthetic weights set no level of their own and their noise-like output reaches a threshold
    far under its peak within the first samples of every row; None keeps the trim_db of **kw (default -40)."""
    from hifigan.longform import LongForm
    lf = LongForm(tts["m"], tts["g"], tts["den"], output, n_timesteps=2, pause_ms=12.0, fade_ms=2.0, head_ms=1.0,
                  tail_ms=3.0, trim_pad_ms=1.0, **kw)
    seg, lens, doc_first = lf.segments(tts["docs"], seeds=tts["seeds"])
    if under_peak_db is not None:
        peak = float(seg.abs().max())
        assert peak > 0 and math.isfinite(peak)
        lf.trim_db = min(20.0 * math.log10(peak) - under_peak_db, 0.0)
    return lf, seg, lens, doc_first


def test_longform_equals_the_specification_on_its_own_segments(tts):
    from hifigan.output import AudioOutput
    output = AudioOutput(16000, loudness=-16, encoding="pcm16")
    lf, seg, lens, doc_first = _longform(tts, output)
    S, L = seg.shape
    assert S == 6 and doc_first.tolist() == [0, 3, 6] and lens.dtype == torch.int32 and int(lens.min()) > 0
    pauses = [[12.0, -4.0], None]                        # a crossfade of 4 ms inside document 0
    doc = lf(tts["docs"], pauses=pauses, seeds=tts["seeds"])
    # the specification on exactly these rows
    seg_np, lens_np = _np(seg), _np(lens)
    thr = 10.0 ** (lf.trim_db / 20.0)
    edges = [jn.edges_ref(seg_np[s], int(lens_np[s]), thr, lf.pad) for s in range(S)]
    start, end = [e[0] for e in edges], [e[1] for e in edges]
    print(f"valid samples {lens_np.tolist()}, trim edges {edges}")
    assert any(e > a for a, e in edges)                  # the loudest sample is kept, whatever else is
    assert any((a, e) != (0, int(n)) for (a, e), n in zip(edges, lens_np))   # and the trim cut something
    gap = [192, -64, 0, 192, 192, 0]
    assert lf._gaps(pauses, [0, 3, 6]) == gap and (lf.fade, lf.head, lf.tail, lf.pad) == (32, 16, 48, 16)
    dst, doc_len, bad = jn.plan_ref([0, 3, 6], start, end, gap, lf.head, lf.tail, L)
    assert bad == 0
    want = jn.join_ref(seg_np, start, end, [0, 3, 6], dst, doc_len, lf.fade)
    fin = output.finish(torch.from_numpy(want).to(DEV), _i32(doc_len))
    assert doc.audio.dtype == torch.int16 and doc.sample_rate == 16000
    assert np.array_equal(_np(doc.lengths), doc_len) and doc.lengths.dtype == torch.int32
    assert torch.equal(doc.audio, fin.audio) and torch.equal(doc.gain, fin.gain)
    table = np.stack([[0, 0, 0, 1, 1, 1], dst, dst + (np.asarray(end) - np.asarray(start))], axis=1)
    assert doc.segments.dtype == torch.int32 and np.array_equal(_np(doc.segments), table)
    assert int(doc.audio.abs().max()) > 0
    # trim_db = None keeps whole sentences
    lf.trim_db = None
    whole = lf(tts["docs"], pauses=pauses, seeds=tts["seeds"])
    d0, l0, _ = jn.plan_ref([0, 3, 6], [0] * S, lens_np, gap, lf.head, lf.tail, L)
    assert np.array_equal(_np(whole.lengths), l0) and np.array_equal(_np(whole.segments)[:, 1], d0)


def test_longform_does_not_depend_on_the_batching(tts):
    """max_batch = 1 and 32 give the same lengths and sentence table, at the default trim_db and with trim_db=None.
    Bytes are compared only when `segments` is first found bit-equal between the two batchings. On the MI355X with
    these weights it is not (printed below): a sentence whose batch pads it to another frame count gets another mel
    (up to 6.6 in log-mel units here), the reference's own GroupNorm-over-padding behaviour, and the
    vocoder, denoiser and resampler are bit-stable on equal mels. The documents' bytes are then left uncompared; no
    tolerance stands in. The table is equal because the frame counts are exact and, at -40 dB, the noise-like output
    of synthetic weights is trimmed nowhere; a trim that cuts follows the audio and with it the batching."""
    from hifigan.output import AudioOutput
    output = AudioOutput(16000, loudness=-16, encoding="pcm16")
    lf32, seg32, lens32, _ = _longform(tts, output, under_peak_db=None, max_batch=32)
    lf1, seg1, lens1, _ = _longform(tts, output, under_peak_db=None, max_batch=1)
    assert lf1.trim_db == lf32.trim_db == -40.0 and torch.equal(lens1, lens32)
    n = min(seg1.shape[1], seg32.shape[1])
    stable = torch.equal(seg1[:, :n], seg32[:, :n]) and not seg1[:, n:].any() and not seg32[:, n:].any()
    print(f"synthesize .. resample bit-stable across max_batch 1 / 32: {stable}")
    for trim_db in (-40.0, None):
        lf1.trim_db = lf32.trim_db = trim_db
        a = lf32(tts["docs"], seeds=tts["seeds"])
        b = lf1(tts["docs"], seeds=tts["seeds"])
        assert torch.equal(a.lengths, b.lengths) and torch.equal(a.segments, b.segments)
        if stable:
            assert torch.equal(a.audio, b.audio) and torch.equal(a.gain, b.gain)


def test_peak_normalisation_is_per_document(tts):
    """With normalize="peak" the document's peak becomes `level`: the gain is fl32(level / peak) (relative error at
    most 2^-24) and the product with the peak sample rounds once more (2^-24), so the delivered peak is within
    2^-23 (1 + 2^-24) relative of level. No single sentence sets the gain: the sentences' own peaks stay apart."""
    from hifigan.output import AudioOutput
    output = AudioOutput(16000, normalize="peak")
    lf, *_ = _longform(tts, output)
    doc = lf(tts["docs"], seeds=tts["seeds"])
    assert doc.audio.dtype == torch.float32
    level = output.level
    sent_peaks = []
    for d in range(2):
        n = int(doc.lengths[d])
        peak = float(doc.audio[d, :n].abs().max())
        print(f"document {d}: peak {peak!r}, gain {float(doc.gain[d])!r}")
        assert abs(peak - level) <= level * 2.0 ** -23 * (1 + 2.0 ** -24)
        assert not doc.audio[d, n:].any()
    for d, lo, hi in doc.segments.tolist():
        if hi > lo:
            sent_peaks.append(float(doc.audio[d, lo:hi].abs().max()))
    print(f"sentence peaks {sent_peaks}")
    assert max(sent_peaks) <= level * (1 + 2.0 ** -23) and min(sent_peaks) < max(sent_peaks)
