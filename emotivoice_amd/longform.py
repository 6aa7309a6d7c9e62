"""Host side of long-form synthesis (``EVEngine.synthesize_long`` / ``EVEngine.stitch``; ev_stitch, include/evhip.h): splitting a text into
sentences with a pause class per joint, the pause table, the stitching configuration in milliseconds, and the per-segment arrays of one call.

The reference synthesises one utterance per input line and stops there ("Support longer text" is the open item of its roadmap), so nothing here
restates it except ``trim_frac = 0.005``, the value of ``prompt_dataset.get_mel``'s trim.  The defaults -- the threshold, the 10 ms kept around a
cut, the 5 ms fades and the pause table -- are starting values: NOBODY HAS MEASURED THEM ON A RELEASED CHECKPOINT, by ear or otherwise.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _ffi
from ._ffi import EV_STITCH_MAX_DOC as MAX_DOC
from ._ffi import EV_STITCH_MAX_FADE as MAX_FADE
from ._ffi import EV_STITCH_MAX_PAUSE as MAX_PAUSE

SENTENCE_END = "。！？；.!?;"
CLAUSE_END = "，、,:"
_CLOSERS = "\"'”’）)」』】》]"
_ASCII_ENDS = ".!?;,:"
PAUSE_CLASSES = ("none", "comma", "sentence", "paragraph")      # ascending: where two boundaries meet, the larger class stays

# pause class -> milliseconds of silence between two sentences; a negative value is a cross-fade of that length (clamped by ev_stitch_plan).
# Not measured on a released checkpoint (see the module docstring).
pauses_ms: Dict[str, float] = {"none": 0.0, "comma": 120.0, "sentence": 300.0, "paragraph": 600.0}


@dataclass
class StitchConfig:
    """ev_stitch_config in milliseconds; ``keep`` / ``fade`` / ``lead`` / ``tail`` in samples override their ``*_ms`` twins when given.  The
    defaults cut what lies below 0.5 % of a sentence's peak (the reference's get_mel value), keep 10 ms around the cut and fade 5 ms at every
    free end.  They have not been measured on a released checkpoint."""
    sample_rate: int = 16000
    trim_frac: float = 0.005
    trim_abs: float = 0.0
    keep_ms: float = 10.0
    fade_ms: float = 5.0
    lead_ms: float = 0.0
    tail_ms: float = 0.0
    keep: Optional[int] = None
    fade: Optional[int] = None
    lead: Optional[int] = None
    tail: Optional[int] = None
    want_int16: bool = False

    def samples(self, name: str) -> int:
        v = getattr(self, name)
        if v is not None:
            return int(v)
        ms = float(getattr(self, name + "_ms"))
        if not math.isfinite(ms):
            raise ValueError("%s_ms %r is not finite" % (name, ms))
        return int(round(ms * self.sample_rate / 1000.0))

    def validate(self) -> "StitchConfig":
        """The rejections of ev_stitch that concern the configuration, with messages that name the field."""
        if int(self.sample_rate) < 1:
            raise ValueError("sample_rate %d must be positive" % self.sample_rate)
        tf, ta = float(self.trim_frac), float(self.trim_abs)
        if not math.isfinite(tf) or tf < 0.0 or not tf < 1.0:
            raise ValueError("trim_frac %r outside [0, 1)" % (self.trim_frac,))
        if not math.isfinite(ta) or ta < 0.0:
            raise ValueError("trim_abs %r must be finite and >= 0" % (self.trim_abs,))
        for name in ("keep", "lead", "tail"):
            if not 0 <= self.samples(name) < 2 ** 31:
                raise ValueError("%s = %d samples must be >= 0" % (name, self.samples(name)))
        if not 0 <= self.samples("fade") <= MAX_FADE:
            raise ValueError("fade = %d samples outside [0, EV_STITCH_MAX_FADE %d]" % (self.samples("fade"), MAX_FADE))
        return self

    def to_struct(self) -> _ffi.ev_stitch_config:
        self.validate()
        c = _ffi.ev_stitch_config()
        c.struct_size = C.sizeof(_ffi.ev_stitch_config)
        c.trim_frac, c.trim_abs = float(self.trim_frac), float(self.trim_abs)
        c.keep, c.fade, c.lead, c.tail = (self.samples(k) for k in ("keep", "fade", "lead", "tail"))
        c.want_i16 = 1 if self.want_int16 else 0
        return c


def _ends_here(text: str, i: int, marks: str) -> bool:
    """text[i] is one of ``marks`` and ends a piece there.  An ASCII mark only does before white space, the end, or a character that is neither an
    ASCII letter nor a digit ("3.14", "a.m", "12:30" stay whole)."""
    ch = text[i]
    if ch not in marks:
        return False
    if ch in _ASCII_ENDS and i + 1 < len(text):
        nx = text[i + 1]
        if nx.isascii() and nx.isalnum():
            return False
    return True


def _closes_here(text: str, j: int) -> bool:
    """text[j] is a closing quote or bracket; a straight quote only counts before white space or the end (elsewhere it may open the next piece)."""
    if text[j] not in _CLOSERS:
        return False
    return text[j] not in "\"'" or j + 1 == len(text) or text[j + 1].isspace()


def _cut(text: str, marks: str) -> List[str]:
    """``text`` cut after every run of ``marks`` (with the other end marks and closing quotes that follow it); the cuts joined give ``text``."""
    out, start, i = [], 0, 0
    while i < len(text):
        if _ends_here(text, i, marks):
            j = i + 1
            while j < len(text) and (_closes_here(text, j) or _ends_here(text, j, SENTENCE_END + CLAUSE_END)):
                j += 1
            out.append(text[start:j])
            start = i = j
        else:
            i += 1
    if start < len(text):
        out.append(text[start:])
    return out


def _pack(parts: Sequence[str], max_chars: int) -> List[str]:
    """Consecutive parts joined greedily while the stripped result stays within ``max_chars``."""
    out, cur = [], ""
    for p in parts:
        if cur.strip() and len((cur + p).strip()) > max_chars:
            out.append(cur)
            cur = p
        else:
            cur += p
    if cur:
        out.append(cur)
    return out


def _hard_split(piece: str, max_chars: int) -> List[str]:
    """A clause longer than ``max_chars``: at white space where there is some, else every ``max_chars`` characters."""
    words = piece.split()
    out: List[str] = []
    for chunk in _pack([w + " " for w in words], max_chars):
        chunk = chunk.strip()
        out.extend(chunk[k:k + max_chars] for k in range(0, len(chunk), max_chars))
    return out


def split_text(text: str, max_chars: int = 80) -> Tuple[List[str], List[str]]:
    """``text`` -> (pieces, joints): the sentences in order and, for each of the len(pieces) - 1 joints, its pause class (a key of ``pauses_ms``).

    A piece ends after 。！？；.!?; (class "sentence") or at a newline ("paragraph"); a sentence longer than ``max_chars`` is cut further after
    ，、,: ("comma"), and a clause that is still too long at white space or, as the last resort, every ``max_chars`` characters ("none").  Every
    piece keeps its punctuation, is stripped of the white space around it, is never empty and never longer than ``max_chars``; the pieces joined
    give the text back up to the white space dropped at the joints."""
    if max_chars < 1:
        raise ValueError("max_chars %d must be >= 1" % max_chars)
    rank = {c: i for i, c in enumerate(PAUSE_CLASSES)}
    pieces: List[str] = []
    joints: List[str] = []
    pending = "none"          # the class of the boundary in front of the next piece

    def emit(piece: str, boundary_after: str):
        nonlocal pending
        piece = piece.strip()
        if piece:
            if pieces:
                joints.append(pending)
            pieces.append(piece)
            pending = boundary_after
        elif rank[boundary_after] > rank[pending]:
            pending = boundary_after

    for line in text.splitlines():
        for sentence in _cut(line, SENTENCE_END):
            if len(sentence.strip()) <= max_chars:
                emit(sentence, "sentence")
                continue
            groups = _pack(_cut(sentence, CLAUSE_END), max_chars)
            for gi, group in enumerate(groups):
                after_group = "sentence" if gi == len(groups) - 1 else "comma"
                if len(group.strip()) <= max_chars:
                    emit(group, after_group)
                    continue
                hard = _hard_split(group, max_chars)
                for hi, hpiece in enumerate(hard):
                    emit(hpiece, after_group if hi == len(hard) - 1 else "none")
        if pieces and rank["paragraph"] > rank[pending]:
            pending = "paragraph"
    return pieces, joints


Pause = Union[str, float, int, None]


def pause_samples(pause: Pause, sample_rate: int = 16000, table: Optional[Dict[str, float]] = None) -> int:
    """A pause class (a key of ``table``, default ``pauses_ms``), a number of milliseconds (negative: a cross-fade) or None (0) -> samples."""
    if pause is None:
        return 0
    if isinstance(pause, str):
        t = pauses_ms if table is None else table
        if pause not in t:
            raise ValueError("unknown pause class %r (known: %s)" % (pause, ", ".join(sorted(t))))
        pause = t[pause]
    ms = float(pause)
    if not math.isfinite(ms):
        raise ValueError("pause %r is not finite" % (pause,))
    return int(round(ms * sample_rate / 1000.0))


def plan_document(seg_doc: Sequence[int], pauses: Sequence[Pause], sample_rate: int = 16000,
                  table: Optional[Dict[str, float]] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The per-segment arrays of one ev_stitch call: (seg_doc int32 (S,), pause_after int32 (S,)).  ``seg_doc``: the document of every segment,
    non-decreasing from 0 without gaps; ``pauses``: one entry per segment (the pause after it: a class, milliseconds or None); the entry of a
    document's last segment is ignored and stored as 0.  Raises for what ev_stitch would reject."""
    sd = np.ascontiguousarray(seg_doc, np.int64).reshape(-1)
    S = sd.size
    if not 1 <= S <= 65535:
        raise ValueError("S %d outside [1, 65535]" % S)
    if len(pauses) != S:
        raise ValueError("%d pauses for %d segments" % (len(pauses), S))
    if sd[0] != 0 or ((np.diff(sd) != 0) & (np.diff(sd) != 1)).any():
        raise ValueError("seg_doc must start at 0 and never decrease or skip a document")
    pa = np.zeros(S, np.int32)
    for s in range(S - 1):
        if sd[s + 1] != sd[s]:
            continue
        v = pause_samples(pauses[s], sample_rate, table)
        if not -MAX_FADE <= v <= MAX_PAUSE:
            raise ValueError("pause_after[%d] = %d samples outside [-EV_STITCH_MAX_FADE %d, EV_STITCH_MAX_PAUSE %d]" % (s, v, MAX_FADE, MAX_PAUSE))
        pa[s] = v
    return sd.astype(np.int32), pa


def flatten_documents(documents: Sequence) -> Tuple[list, np.ndarray, list]:
    """documents: each a dict(utts=[...], pauses=[...]) or a pair (utts, pauses), ``pauses`` having one entry per joint (len(utts) - 1; None = all
    "sentence") -> (the utts in order, seg_doc, one pause per segment)."""
    utts, seg_doc, pauses = [], [], []
    for d, doc in enumerate(documents):
        u, p = (doc["utts"], doc.get("pauses")) if isinstance(doc, dict) else doc
        if len(u) < 1:
            raise ValueError("document %d has no sentence" % d)
        p = ["sentence"] * (len(u) - 1) if p is None else list(p)
        if len(p) != len(u) - 1:
            raise ValueError("document %d: %d pauses for %d sentences (one per joint)" % (d, len(p), len(u)))
        utts.extend(u)
        seg_doc.extend([d] * len(u))
        pauses.extend(p + [None])
    return utts, np.asarray(seg_doc, np.int32), pauses


def ramp_table(F: int) -> np.ndarray:
    """tab[i] = (float)(0.5 - 0.5 cos(pi (i + 0.5) / F)), computed in float64 and rounded once: the table of ev_stitch_ramp."""
    if not 0 <= F <= MAX_FADE:
        raise ValueError("F %d outside [0, EV_STITCH_MAX_FADE %d]" % (F, MAX_FADE))
    i = np.arange(F, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(np.pi * (i + 0.5) / max(F, 1))).astype(np.float32)


__all__ = ["StitchConfig", "split_text", "pauses_ms", "pause_samples", "plan_document", "flatten_documents", "ramp_table", "PAUSE_CLASSES", "MAX_DOC"]
