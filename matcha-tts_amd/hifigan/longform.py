"""Long-form synthesis: documents (paragraphs, articles, chapters) given as lists of sentences, synthesized as batches
of sentences and joined into one piece of audio per document on the GPU. No counterpart in the reference, whose
main.py writes one file per sentence and leaves trimming, pauses and levelling to the caller.

    lf = LongForm(model, vocoder, denoiser, AudioOutput(16000, loudness=-16.0, encoding="pcm16"))
    doc = lf([[s0, s1, s2], [t0, t1]], seeds=[7, 8])     # two documents of 3 and 2 sentences (int64 token tensors)
    doc.audio[d, :doc.lengths[d]]                        # int16 at 16 kHz, each DOCUMENT at -16 LUFS
    doc.segments                                         # int32 [S, 3]: (document, first sample, end sample)

The sentences of all documents are sorted by token count into batches of at most `max_batch`, run through
synthesize -> vocoder -> denoiser -> the output stage's resampler, and land as fp32 rows of one [S, L] buffer in
document order. One chain follows (matcha_hip/join.py is the specification on the CPU):

    mt_audio_edges -> mt_join_plan -> mt_join -> AudioOutput.finish

the silence round every sentence is trimmed, the sentences are placed with their pauses (a negative pause is a
crossfade), written with raised-cosine fades, and level, normalisation, loudness= and the encoding are applied per
document: a whispered aside stays quieter than the headline. trim_db, pause_ms and fade_ms are interface defaults,
not measured quality claims.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence

import torch

from matcha_hip import join as jn
from matcha_hip import runtime as rt

from .output import AudioOutput

SEED_SHIFT = 20           # sentence j of a document with seed sd draws from (sd << 20) | j
SEED_DOC_MAX = 1 << 43    # sd < 2^43: the sentence seed stays a positive int64


class Document(NamedTuple):
    audio: torch.Tensor          # [D, Ld] in the output encoding
    lengths: torch.Tensor        # int32 [D], valid samples of each document at sample_rate
    sample_rate: int
    gain: torch.Tensor           # fp32 [D], the gain each document was multiplied by
    segments: torch.Tensor       # int32 [S, 3]: (document, first sample, end sample) of every sentence, in order


def _samples(ms: float, rate: int, what: str) -> int:
    ms = float(ms)
    if not math.isfinite(ms):
        raise ValueError(f"{what} must be finite, got {ms}")
    return int(round(ms * rate / 1000.0))


class LongForm:
    """model: MatchaTTS; generator: the HiFi-GAN Generator; denoiser: Denoiser or None; output: the AudioOutput that
    sets rate, level and encoding of the documents. trim_db: a sample at or above this level (dB re full scale, at
    the output rate) is speech, everything before the first and after the last such sample of a sentence, less
    trim_pad_ms, is dropped (None: nothing is trimmed). pause_ms: the silence between two sentences (negative: they
    overlap by that much and crossfade). fade_ms: the raised-cosine fade at both ends of every sentence. head_ms /
    tail_ms: silence before the first and after the last sentence of a document."""

    def __init__(self, model, generator, denoiser, output: AudioOutput, n_timesteps: int = 10, max_batch: int = 32,
                 strength: float = 0.00025, trim_db: Optional[float] = -40.0, trim_pad_ms: float = 20.0,
                 pause_ms: float = 250.0, fade_ms: float = 5.0, head_ms: float = 0.0, tail_ms: float = 0.0):
        if not isinstance(output, AudioOutput):
            raise TypeError("LongForm: output is the AudioOutput that delivers the documents")
        if not (1 <= int(max_batch) <= rt.JOIN_MAX_ROWS):
            raise ValueError(f"max_batch must be in 1..{rt.JOIN_MAX_ROWS}, got {max_batch}")
        if trim_db is not None and not (math.isfinite(float(trim_db)) and float(trim_db) <= 0.0):
            raise ValueError(f"trim_db must be a finite level at or under 0 dB re full scale, or None; got {trim_db}")
        rate = output.sample_rate
        self.model, self.generator, self.denoiser, self.output = model, generator, denoiser, output
        self.n_timesteps, self.max_batch, self.strength = n_timesteps, int(max_batch), float(strength)
        self.trim_db = None if trim_db is None else float(trim_db)
        self.pad = _samples(trim_pad_ms, rate, "trim_pad_ms")
        self.fade = _samples(fade_ms, rate, "fade_ms")
        self.head = _samples(head_ms, rate, "head_ms")
        self.tail = _samples(tail_ms, rate, "tail_ms")
        for name, v in (("trim_pad_ms", self.pad), ("fade_ms", self.fade), ("head_ms", self.head),
                        ("tail_ms", self.tail)):
            if v < 0:
                raise ValueError(f"{name} must not be negative")
        if self.fade > jn.FADE_MAX:
            raise ValueError(f"fade_ms: {self.fade} samples at {rate} Hz, at most {jn.FADE_MAX}")
        self.pause_ms = float(pause_ms)
        _samples(self.pause_ms, rate, "pause_ms")

    # ---- argument handling (host only) ----------------------------------------------------------------------

    @staticmethod
    def _flatten(docs):
        """-> ([(document, sentence index, tokens)] in document order, doc_first list [D + 1])"""
        if not isinstance(docs, (list, tuple)) or len(docs) == 0:
            raise ValueError("LongForm: docs is a non-empty list of documents, each a list of 1-D int64 token tensors")
        flat, first = [], [0]
        for d, doc in enumerate(docs):
            if not isinstance(doc, (list, tuple)):
                raise ValueError(f"LongForm: document {d} is not a list of sentences")
            if len(doc) > (1 << SEED_SHIFT):
                raise ValueError(f"LongForm: document {d} has {len(doc)} sentences, at most 2^{SEED_SHIFT}")
            for j, s in enumerate(doc):
                if not isinstance(s, torch.Tensor) or s.dim() != 1 or s.dtype != torch.int64 or s.numel() == 0:
                    raise ValueError(f"LongForm: sentence {j} of document {d} is not a non-empty 1-D int64 tensor")
                flat.append((d, j, s))
            first.append(len(flat))
        if not flat:
            raise ValueError("LongForm: no sentence in any document")
        if len(flat) > rt.JOIN_MAX_ROWS or len(docs) > rt.JOIN_MAX_ROWS:
            raise ValueError(f"LongForm: {len(flat)} sentences in {len(docs)} documents, at most {rt.JOIN_MAX_ROWS}")
        return flat, first

    @staticmethod
    def _sentence_seeds(seeds, flat, D: int):
        if seeds is None:
            return None
        if isinstance(seeds, torch.Tensor):
            seeds = seeds.tolist()
        if isinstance(seeds, (int, float)) or len(seeds) != D:
            raise ValueError(f"LongForm: seeds holds one integer per document ({D})")
        for sd in seeds:
            if isinstance(sd, bool) or not isinstance(sd, int) or not (0 <= sd < SEED_DOC_MAX):
                raise ValueError(f"LongForm: document seed {sd!r} is not an integer with 0 <= seed < 2^43")
        return [(int(seeds[d]) << SEED_SHIFT) | j for d, j, _ in flat]

    def _gaps(self, pauses, first: Sequence[int]) -> list:
        """-> the gap in samples after every sentence (0 after a document's last one, where the plan ignores it)"""
        rate = self.output.sample_rate
        D = len(first) - 1
        if pauses is not None and len(pauses) != D:
            raise ValueError(f"LongForm: pauses holds one list per document ({D})")
        default = _samples(self.pause_ms, rate, "pause_ms")
        gaps = []
        for d in range(D):
            n = first[d + 1] - first[d]
            if pauses is None or pauses[d] is None:
                gaps += [default] * max(n - 1, 0)
            else:
                if len(pauses[d]) != max(n - 1, 0):
                    raise ValueError(f"LongForm: document {d} has {n} sentences and {len(pauses[d])} pauses; one per "
                                     "sentence boundary is expected")
                gaps += [_samples(p, rate, "pauses") for p in pauses[d]]
            if n > 0:
                gaps.append(0)
        if any(abs(g) >= (1 << 30) for g in gaps):
            raise ValueError("LongForm: a pause of 2^30 samples or more")
        return gaps

    # ---- the stage before the join ----------------------------------------------------------------------------

    @torch.inference_mode()
    def segments(self, docs, seeds=None, spks=None, **synth_kwargs):
        """-> (seg fp32 [S, L], lens int32 [S], doc_first int32 [D + 1]): every sentence synthesized, vocoded,
        denoised and resampled to the output rate, one row each in document order, lens[s] valid samples. spks: one
        speaker id per document. synth_kwargs go to synthesize (temperature, length_scale, ...: values shared by all
        sentences)."""
        flat, first = self._flatten(docs)
        D, S = len(first) - 1, len(flat)
        sent_seeds = self._sentence_seeds(seeds, flat, D)
        if spks is not None:
            spks = torch.as_tensor(spks).reshape(-1).tolist()
            if len(spks) != D:
                raise ValueError(f"LongForm: spks holds one speaker id per document ({D})")
        dev = flat[0][2].device
        rt.require_gpu(*[s for _, _, s in flat], what="LongForm")
        order = sorted(range(S), key=lambda i: flat[i][2].numel())  # stable: equal counts keep document order
        parts = []
        for b0 in range(0, S, self.max_batch):
            idx = order[b0:b0 + self.max_batch]
            toks = [flat[i][2] for i in idx]
            xl = torch.tensor([t.numel() for t in toks], dtype=torch.int64, device=dev)
            x = torch.nn.utils.rnn.pad_sequence(toks, batch_first=True)
            kw = dict(synth_kwargs)
            if sent_seeds is not None:
                kw["seeds"] = torch.tensor([sent_seeds[i] for i in idx], dtype=torch.int64, device=dev)
            if spks is not None:
                kw["spks"] = torch.tensor([spks[flat[i][0]] for i in idx], dtype=torch.int64, device=dev)
            mel, y_lengths, _ = self.model.synthesize(x, xl, self.n_timesteps, **kw)
            wav = self.generator(mel, lengths=y_lengths).squeeze(1)
            if self.denoiser is not None:
                wav = self.denoiser(wav, strength=self.strength, lengths=y_lengths)
            audio, lens = self.output._resampled(wav, y_lengths, "LongForm")
            parts.append((torch.tensor(idx, dtype=torch.int64, device=dev), audio, lens))
        L = max(a.shape[1] for _, a, _ in parts)
        seg = torch.zeros((S, L), dtype=torch.float32, device=dev)
        lens_all = torch.zeros((S,), dtype=torch.int32, device=dev)
        for rows, audio, lens in parts:
            seg[rows, :audio.shape[1]] = audio.to(torch.float32)
            lens_all[rows] = lens.to(torch.int32)
        return seg, lens_all, torch.tensor(first, dtype=torch.int32, device=dev)

    # ---- the join ---------------------------------------------------------------------------------------------

    def edges(self, seg: torch.Tensor, lens: torch.Tensor):
        """-> (start, end) int32 [S] of the rows of `segments`: the trim edges, (0, lens) with trim_db=None"""
        if self.trim_db is None:
            return torch.zeros_like(lens), lens.clamp(0, seg.shape[1]).to(torch.int32)
        return rt.audio_edges(seg, lens, 10.0 ** (self.trim_db / 20.0), self.pad)

    @torch.inference_mode()
    def __call__(self, docs, pauses=None, seeds=None, spks=None, **synth_kwargs) -> Document:
        """docs: a list of documents, each a list of 1-D int64 token tensors on the GPU, one per sentence. pauses:
        per document (or None for pause_ms) one value in ms per sentence boundary; negative means crossfade. seeds:
        one integer per document, 0 <= seed < 2^43: sentence j draws its noise from (seed << 20) | j, whatever batch it
        lands in; None: randn. The join adds no batch dependence of its own; synthesize has one, the reference's: a
        sentence's mel depends on the frame count its batch is padded to, so max_batch can change the
        audio of a sentence, not its length."""
        flat, first = self._flatten(docs)
        gaps = self._gaps(pauses, first)
        self._sentence_seeds(seeds, flat, len(first) - 1)  # refused before any launch
        seg, lens, doc_first = self.segments(docs, seeds=seeds, spks=spks, **synth_kwargs)
        S, L = seg.shape
        dev = seg.device
        start, end = self.edges(seg, lens)
        gap = torch.tensor(gaps, dtype=torch.int32, device=dev)
        dst, doc_len, bad = rt.join_plan(doc_first, start, end, gap, self.head, self.tail, L)
        joined = rt.join(seg, start, end, doc_first, dst, doc_len, self.fade, bad=bad)
        out = self.output.finish(joined, doc_len)
        doc_of = torch.tensor([d for d, _, _ in flat], dtype=torch.int32, device=dev)
        a = start.clamp(0, L)
        n = torch.maximum(end, a).clamp(max=L) - a
        table = torch.stack([doc_of, dst, dst + n], dim=1).contiguous()
        return Document(out.audio, doc_len, self.output.sample_rate, out.gain, table)
