"""Host packing of a batch for the library: segments back to back, utterances as the five arrays of a synthesis call.  numpy only."""
from typing import Callable, Optional, Sequence

import numpy as np


def pack_segments(wavs, name: str = "wavs", min_samples: int = 1, flatten: bool = False, limit: Optional[Callable[[int], Optional[str]]] = None):
    """Waveforms back to back: (flat array, is_int16, lens int64).  All int16 or all floating (converted to float32), at least one of them, each of
    ``min_samples`` or more.  ``flatten``: an array of any shape counts as its samples in order (otherwise only 1-D arrays pass).  ``limit``: the
    caller's own bounds on a segment of n samples, the text of the error or None.  Every error is a ValueError that names the segment."""
    if len(wavs) == 0:
        raise ValueError("%s: no utterances (at least one segment is needed)" % name)
    arrs = [np.asarray(w) for w in wavs]
    is16 = arrs[0].dtype == np.int16
    for b, a in enumerate(arrs):
        why = None
        if a.ndim != 1 and not flatten:
            why = "expected a 1-D array, got shape %s" % (a.shape,)
        elif (a.dtype == np.int16) != is16:
            why = "int16 and floating utterances cannot be mixed in one call"
        elif not is16 and not np.issubdtype(a.dtype, np.floating):
            why = "expected int16 or floating samples, got %s" % a.dtype
        elif a.size < min_samples:
            why = "%d samples < %d" % (a.size, min_samples)
        elif limit is not None:
            why = limit(a.size)
        if why:
            raise ValueError("%s[%d]: %s" % (name, b, why))
    flat = np.ascontiguousarray(np.concatenate([a.reshape(-1).astype(np.int16 if is16 else np.float32, copy=False) for a in arrs]))
    return flat, is16, np.array([a.size for a in arrs], np.int64)


def pack_utts(utts: Sequence[dict]):
    """Utterance dicts (ling, speaker, style, content) -> (ling int64 packed, cu_seqlens int32 (B + 1,), speaker int64 (B,), style and content
    float32 (B, dim)), all contiguous."""
    ling = np.ascontiguousarray(np.concatenate([np.asarray(u["ling"], np.int64) for u in utts]))
    cu = np.zeros(len(utts) + 1, np.int32)
    cu[1:] = np.cumsum([len(u["ling"]) for u in utts])
    spk = np.ascontiguousarray([int(u["speaker"]) for u in utts], np.int64)
    style = np.ascontiguousarray(np.stack([np.asarray(u["style"], np.float32) for u in utts]))
    content = np.ascontiguousarray(np.stack([np.asarray(u["content"], np.float32) for u in utts]))
    return ling, cu, spk, style, content
