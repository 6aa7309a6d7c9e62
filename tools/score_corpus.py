#!/usr/bin/env python3
"""Objective scores of a checkpoint against recordings: synthesises every line of a text file in the reference's format
(``speaker|prompt|phonemes|content``) and scores it against the recording of the same line, on the device (emotivoice_amd.scoring.score_recordings:
MCD along the DTW path, F0 RMSE / bias in cents, voiced / unvoiced error).  One JSON line per utterance, then one for the corpus.

    python tools/score_corpus.py -c <config_folder> --checkpoint <generator checkpoint> -t <text file> --wavs <dir> [--out scores.jsonl]

Recordings are ``<dir>/<line number>.wav`` (1-based, the names inference_am_vocoder_joint writes), 16-bit PCM at any rate ev_resample takes.  The MCD
is an MFCC-style one on the engine's own log-mel and the F0 tracks are YIN's: the figures compare among themselves only."""
import argparse
import json
import os
import sys
import wave

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def read_wav(path):
    """(int16 mono samples, sample rate) of a 16-bit PCM file; further channels are dropped."""
    import numpy as np
    with wave.open(path, "rb") as w:
        if w.getsampwidth() != 2:
            raise ValueError("%s: %d-byte samples; 16-bit PCM expected" % (path, w.getsampwidth()))
        x = np.frombuffer(w.readframes(w.getnframes()), np.int16).reshape(-1, w.getnchannels())
        return np.ascontiguousarray(x[:, 0]), w.getframerate()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-c", "--config_folder", required=True)
    ap.add_argument("--checkpoint", default="", help="a generator checkpoint (torch.load(...)['generator'])")
    ap.add_argument("--synthetic-weights", action="store_true", help="no checkpoint: the seeded synthetic one (a dry run of the tool)")
    ap.add_argument("-t", "--test_file", required=True)
    ap.add_argument("--wavs", required=True, help="directory of <line number>.wav recordings")
    ap.add_argument("--embeddings", default=None, help=".npz with 'style' and 'content' (n_lines, 768) arrays; default: the placeholder embedder")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--n-ceps", type=int, default=13)
    ap.add_argument("--trim", action="store_true", help="trim the recordings' leading and trailing silence as the reference's get_mel does")
    ap.add_argument("--precision", default="mx", choices=["mx", "fast", "strict"])
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default="-", help="JSON lines; - = stdout")
    args = ap.parse_args(argv)

    import numpy as np

    from emotivoice_amd.config import load_yaml
    from emotivoice_amd.generator import JETSGeneratorHIP
    from emotivoice_amd.inference_am_vocoder_joint import _load_config
    from emotivoice_amd.scoring import ScoreConfig, corpus_means, score_recordings
    from emotivoice_amd.text_io import HashStyleEmbedder, phonemes_to_ids, read_table, read_text_file

    config = _load_config(args.config_folder)
    conf = load_yaml(config.model_config_path, n_vocab=config.n_symbols, n_speaker=config.speaker_n_labels)
    token2id, speaker2id = read_table(config.token_list_path), read_table(config.speaker2id_path)
    gen = JETSGeneratorHIP(conf, precision=args.precision)
    shapes = gen.shapes
    if args.synthetic_weights:
        from emotivoice_amd.synthetic import synth_state_dict
        sd = synth_state_dict(0, "parity", shapes)
    elif args.checkpoint:
        import torch
        sd = torch.load(args.checkpoint, map_location="cpu")["generator"]
    else:
        ap.error("--checkpoint or --synthetic-weights is required")
    emb = np.load(args.embeddings) if args.embeddings else None
    embedder = HashStyleEmbedder(shapes.bert_dim)
    todo = []
    for i, ln in enumerate(read_text_file(args.test_file)):
        path = os.path.join(args.wavs, "%d.wav" % (i + 1))
        if ln.speaker not in speaker2id or not os.path.exists(path):
            continue
        utt = dict(ling=phonemes_to_ids(ln.phonemes, token2id), speaker=speaker2id[ln.speaker],
                   style=emb["style"][i] if emb is not None else embedder(ln.prompt), content=emb["content"][i] if emb is not None else embedder(ln.content))
        todo.append((i + 1, utt, path))
    if not todo:
        sys.exit("no line of %s has both a known speaker and a recording in %s" % (args.test_file, args.wavs))
    gen.to(args.device).load_state_dict(sd)
    eng = gen._ensure_engine()
    fh = sys.stdout if args.out == "-" else open(args.out, "w")
    rows = []
    try:
        by_rate = {}
        for line_no, utt, path in todo:
            wav, sr = read_wav(path)
            by_rate.setdefault(sr, []).append((line_no, utt, wav))
        for sr, items in sorted(by_rate.items()):
            for s in range(0, len(items), args.batch):
                chunk = items[s:s + args.batch]
                rep = score_recordings(eng, [u for _, u, _ in chunk], [w for _, _, w in chunk], sample_rate=sr, trim=args.trim,
                                       config=ScoreConfig(n_ceps=args.n_ceps))
                for (line_no, _, _), u in zip(chunk, rep["utterances"]):
                    u = dict(line=line_no, sample_rate=sr, **u)
                    rows.append(u)
                    fh.write(json.dumps(u) + "\n")
        fh.write(json.dumps(dict(corpus=corpus_means({k: np.array([r[k] for r in rows]) for k in rows[0] if k not in ("line", "sample_rate")}),
                                 n_ceps=args.n_ceps, trim=bool(args.trim), precision=args.precision)) + "\n")
    finally:
        if fh is not sys.stdout:
            fh.close()
        gen.close()


if __name__ == "__main__":
    main()
