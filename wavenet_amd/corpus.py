"""A training corpus resident on the device, and batches of crops drawn uniformly over ALL its training windows.

The per-file loop of ``train_audio.train`` (``_Crops``) trains ``--repeat`` updates on crops of one file, so a batch holds one
file and one speaker.  ``Corpus`` packs every file's tokens back to back -- uint8 when ``quantization_steps`` <= 256, int32
above -- with its feature columns and class id, uploads them once, and assembles a batch whose crops each come from any file
in ONE launch (``wn_corpus_gather``, include/wavenet_corpus.h).  Each crop carries its own file's class id, feature columns
and phase; what it holds is, value for value, what ``_Crops`` makes of that file on its own: the ``input_width`` silence tokens
in front, ``local.padded`` (column 0 repeated in front) and ``local.with_extra_column`` plus ``_Crops``' clamp (the last
column repeated behind) are index arithmetic in the kernel, never arrays.

The draw rule (``draw_indices``): one ``rng.randint(0, total_windows, size=batch_size)`` call, mapped through the cumulative
window counts of the files to (file, start).  Every training window of the corpus is equally likely, so a long file gets
proportionally more crops; with ONE file the call is ``_Crops.draw``'s own, argument for argument, and one seed selects the
same crops as the per-file loop.  The starts are drawn on the host, so the host knows every crop's phase."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from .wavenet import coarse_frames_needed

CROPS = ("frame", "sample")


def silence_token(quantization_steps: int) -> int:
    """The token training pads a file with (train.py:53)."""
    return 127 if quantization_steps > 127 else quantization_steps // 2


def columns_per_crop(input_width: int, target_width: int, hop: int, crop: str = "frame", interp: str = "repeat",
                     upsample: int = 1) -> int:
    """The feature columns a crop carries, by ``_Crops``' rule: what input_width + target_width positions span from a column
    border (``frame``) or from the worst phase (``sample``), one more for linear interpolation; with a learned upsampling
    layer (``upsample`` > 1) what ``coarse_frames_needed`` asks for."""
    if crop not in CROPS:
        raise Exception("crop must be 'frame' or 'sample', got %r" % (crop,))
    if int(upsample) > 1:
        return coarse_frames_needed(input_width + target_width, hop, upsample, None if crop == "sample" else 0, interp)
    worst = hop - 1 if crop == "sample" else 0
    return (input_width + target_width + worst + hop - 1) // hop + int(interp == "linear")


def check_shard(shard, batch_size: int):
    """(lo, hi) with 0 <= lo < hi <= batch_size, as ints: the crops of a global draw that one rank gathers."""
    lo, hi = int(shard[0]), int(shard[1])
    if not (0 <= lo < hi <= int(batch_size)):
        raise ValueError("shard = (%d, %d) is no range of crops of a batch of %d" % (lo, hi, int(batch_size)))
    return lo, hi


class Corpus(object):
    """``Corpus(tokens_per_file, input_width, quantization_steps, device, features=None, hop=0, classes=None)``.

    ``tokens_per_file``: one 1-D integer array per file (``data.load_audio_file``); ``features``: one float (F, cols_f) array
    per file with at least ceil(len_f / hop) columns (surplus columns are kept: the clamp then reaches them, as it does in the
    per-file path); ``classes``: one class id per file.  Everything is packed and uploaded once; the packed host arrays stay
    (``tokens``, ``features``, ``file_offset`` ...) for inspection and for the tests' reference."""

    def __init__(self, tokens_per_file: Sequence, input_width: int, quantization_steps: int, device, features=None, hop: int = 0,
                 classes=None):
        import torch
        files = [np.asarray(t).reshape(-1) for t in tokens_per_file]
        if not files:
            raise ValueError("Corpus: no file")
        self.input_width, self.quantization_steps = int(input_width), int(quantization_steps)
        if self.input_width < 1:
            raise ValueError("Corpus: input_width = %d < 1" % self.input_width)
        self.device = torch.device(device)
        self.silence = silence_token(self.quantization_steps)
        dtype = np.uint8 if self.quantization_steps <= 256 else np.int32
        for n, t in enumerate(files):
            if t.dtype.kind not in "iu":
                raise ValueError("Corpus: file %d holds %s, tokens are integers" % (n, t.dtype))
            if t.size and (int(t.min()) < 0 or int(t.max()) >= self.quantization_steps):
                raise ValueError("Corpus: file %d holds a token outside [0, %d)" % (n, self.quantization_steps))
            if t.size >= 2 ** 31:
                raise ValueError("Corpus: file %d has %d tokens, a file holds fewer than 2^31" % (n, t.size))
        self.n_files = len(files)
        self.file_len = np.array([t.size for t in files], dtype=np.int32)
        self.file_offset = np.concatenate([[0], np.cumsum(self.file_len.astype(np.int64))[:-1]]).astype(np.int64)
        self.tokens = np.concatenate(files).astype(dtype) if int(self.file_len.sum()) else np.zeros((0,), dtype)
        self.file_class = None
        if classes is not None:
            self.file_class = np.asarray(list(classes), dtype=np.int64)
            if self.file_class.shape != (self.n_files,):
                raise ValueError("Corpus: %d class ids for %d files" % (self.file_class.size, self.n_files))
        self.features = self.col_offset = self.col_count = None
        self.F, self.hop, self.pad_cols, self.shift = 0, 0, 0, 0
        if features is not None:
            feats = [np.asarray(a) for a in features]
            self.hop = int(hop)
            if self.hop < 1:
                raise ValueError("Corpus: hop = %d < 1 with features" % self.hop)
            if len(feats) != self.n_files:
                raise ValueError("Corpus: %d feature arrays for %d files" % (len(feats), self.n_files))
            self.F = int(feats[0].shape[0]) if feats[0].ndim == 2 else 0
            for n, a in enumerate(feats):
                need = max(1, (int(self.file_len[n]) + self.hop - 1) // self.hop)
                if a.ndim != 2 or a.shape[0] != self.F or self.F < 1 or a.shape[1] < need:
                    raise ValueError("Corpus: the features of file %d have shape %s; its %d tokens need (%d, >= %d) at hop %d"
                                     % (n, tuple(a.shape), int(self.file_len[n]), self.F, need, self.hop))
            self.col_count = np.array([a.shape[1] for a in feats], dtype=np.int32)
            self.col_offset = np.concatenate([[0], np.cumsum(self.col_count.astype(np.int64))[:-1]]).astype(np.int64)
            self.features = np.ascontiguousarray(np.concatenate(feats, axis=1), dtype=np.float32)
            self.pad_cols = (self.input_width + self.hop - 1) // self.hop
            self.shift = self.pad_cols * self.hop - self.input_width
        self.last_draw = None
        self.launches = 0
        self._d, self.desc = None, None
        if self.device.type != "cpu":            # (a corpus on "cpu" serves the draw rule and the refusals; it cannot gather)
            self._upload()

    def _upload(self):
        import torch
        from . import _corpus

        def up(a):
            return None if a is None else torch.as_tensor(a).to(self.device)
        # (an empty corpus still gets a one-element token buffer: the descriptor refuses NULL, windows() refuses the draw)
        self._d = dict(tokens=up(self.tokens if self.tokens.size else np.zeros((1,), self.tokens.dtype)),
                       file_offset=up(self.file_offset), file_len=up(self.file_len), file_class=up(self.file_class),
                       features=up(self.features), col_offset=up(self.col_offset), col_count=up(self.col_count))
        self.desc = _corpus.WnCorpusDesc(
            total_cols=0 if self.features is None else int(self.features.shape[1]), n_files=self.n_files,
            token_bytes=self.tokens.dtype.itemsize, F=self.F, hop=self.hop, input_width=self.input_width, silence=self.silence,
            pad_cols=self.pad_cols, shift=self.shift, **{k: (None if v is None else v.data_ptr()) for k, v in self._d.items()})

    # -- the draw rule, on the host -----------------------------------------------------------------------------------------------
    def _frame_offset(self) -> int:
        return (-self.shift) % self.hop                      # the first start whose position lies on a column border

    def _mode(self, crop: str) -> str:
        if crop not in CROPS:
            raise Exception("crop must be 'frame' or 'sample', got %r" % (crop,))
        return "sample" if self.features is None else crop

    def windows(self, target_width: int, crop: str = "sample") -> np.ndarray:
        """Training windows per file (int64): a file with none is left out of the draw.  ``hi_f = len_f - target_width - 1`` is
        ``_Crops``' ``hi`` on the padded signal; ``sample`` (or no features): max(hi_f, 0) starts 0 .. hi_f - 1; ``frame``: the
        starts r, r + hop, ... below hi_f, r the first index on a column border."""
        hi = self.file_len.astype(np.int64) - int(target_width) - 1
        if self._mode(crop) == "sample":
            return np.maximum(hi, 0)
        r = self._frame_offset()
        return np.where(hi - r > 0, (hi - r + self.hop - 1) // self.hop, 0)

    def draw_indices(self, batch_size: int, target_width: int, crop: str = "sample", rng=np.random):
        """-> (files, starts), one (file, start) per crop, from ONE ``rng.randint(0, total_windows, size=batch_size)`` call."""
        counts = self.windows(target_width, crop)
        total = int(counts.sum())
        if total < 1:
            raise Exception("signal too short for input_width + train_width: no file of the corpus has a training window")
        g = rng.randint(0, total, size=batch_size)
        ends = np.cumsum(counts)
        files = np.searchsorted(ends, g, side="right")
        k = g - (ends[files] - counts[files])
        starts = k if self._mode(crop) == "sample" else self._frame_offset() + self.hop * k
        return files.astype(np.int64), starts.astype(np.int64)

    def phases(self, starts) -> Optional[np.ndarray]:
        """(start + shift) % hop of every crop (int32), None without features."""
        if self.features is None:
            return None
        return ((np.asarray(starts, dtype=np.int64) + self.shift) % self.hop).astype(np.int32)

    # -- the gather, on the device ------------------------------------------------------------------------------------------------
    def check_draws(self, files, starts, target_width: int):
        """Refuse, naming the crop, what the kernel would only fence: a file index or start out of range, a left-out file."""
        files, starts = np.asarray(files), np.asarray(starts)
        if files.ndim != 1 or files.shape != starts.shape or files.size < 1 or files.dtype.kind not in "iu" or starts.dtype.kind not in "iu":
            raise ValueError("Corpus.gather: files and starts are two integer arrays of one length >= 1, got %s %s and %s %s"
                             % (files.dtype, tuple(files.shape), starts.dtype, tuple(starts.shape)))
        if int(target_width) < 1:
            raise ValueError("Corpus.gather: target_width = %d < 1" % int(target_width))
        files, starts = files.astype(np.int64), starts.astype(np.int64)
        bad = np.flatnonzero((files < 0) | (files >= self.n_files))
        if bad.size:
            raise ValueError("Corpus.gather: crop %d names file %d; the corpus has files 0 .. %d"
                             % (int(bad[0]), int(files[bad[0]]), self.n_files - 1))
        hi = self.file_len.astype(np.int64)[files] - int(target_width) - 1
        out = np.flatnonzero(hi <= 0)
        if out.size:
            b = int(out[0])
            raise ValueError("Corpus.gather: crop %d names file %d, which is left out: its %d tokens hold no window of "
                             "target_width %d" % (b, int(files[b]), int(self.file_len[files[b]]), int(target_width)))
        bad = np.flatnonzero((starts < 0) | (starts >= hi))
        if bad.size:
            b = int(bad[0])
            raise ValueError("Corpus.gather: crop %d starts at %d; file %d allows starts 0 .. %d at target_width %d"
                             % (b, int(starts[b]), int(files[b]), int(hi[b]) - 1, int(target_width)))
        return files, starts

    def gather(self, files, starts, target_width: int, n_cols: Optional[int] = None):
        """-> (x (B, input_width + target_width) int32, tgt (B, target_width) int32, local (B, F, n_cols) float32 or None,
        condition (B,) int64 or None, phases (B,) int32 numpy or None).  One H2D copy of the (B, 2) draw table, one launch."""
        import torch
        from . import _corpus, _lib
        files, starts = self.check_draws(files, starts, target_width)
        B, tw = int(files.size), int(target_width)
        if self.features is not None and (n_cols is None or int(n_cols) < 1):
            raise ValueError("Corpus.gather: n_cols = %r; a corpus with features needs the column count per crop (columns_per_crop)"
                             % (n_cols,))
        n_cols = int(n_cols) if self.features is not None else 0
        if self.desc is None:
            raise ValueError("Corpus.gather: this corpus lives on %s; the gather runs on a HIP device" % (self.device,))
        with torch.cuda.device(self.device):
            draws = torch.as_tensor(np.stack([files, starts], axis=1).astype(np.int32)).to(self.device)
            x = torch.empty((B, self.input_width + tw), dtype=torch.int32, device=self.device)
            tgt = torch.empty((B, tw), dtype=torch.int32, device=self.device)
            local = None if self.features is None else torch.empty((B, self.F, n_cols), dtype=torch.float32, device=self.device)
            cond = None if self.file_class is None else torch.empty((B,), dtype=torch.int64, device=self.device)
            _corpus.check(_corpus.lib().wn_corpus_gather(self.desc, _lib.ptr(draws), B, tw, n_cols, _lib.ptr(x), _lib.ptr(tgt),
                                                         _lib.ptr(local), _lib.ptr(cond), _lib.stream_ptr()))
        self.launches += 1
        return x, tgt, local, cond, self.phases(starts)

    def draw(self, batch_size: int, target_width: int, crop: str = "sample", n_cols: Optional[int] = None, rng=np.random,
             shard=None):
        """``gather(*draw_indices(...))``; the (files, starts) drawn stay in ``last_draw``.  ``shard`` = (lo, hi), a rank of a
        data-parallel run: the draw is the global one all the same -- ``batch_size`` pairs from the one ``randint`` call, all of
        them kept in ``last_draw`` -- and crops lo .. hi - 1 of it are gathered, so equally seeded ranks cover one global batch."""
        files, starts = self.draw_indices(batch_size, target_width, crop, rng)
        self.last_draw = (files, starts)
        if shard is not None:
            lo, hi = check_shard(shard, batch_size)
            files, starts = files[lo:hi], starts[lo:hi]
        return self.gather(files, starts, target_width, n_cols)

    def device_bytes(self) -> int:
        return sum(int(v.numel()) * v.element_size() for v in self._d.values() if v is not None)
