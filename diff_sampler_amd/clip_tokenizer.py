"""The CLIP byte-pair tokenizer, host only: prompts -> the [B, 77] token ids ``clip_engine.ClipTextEncoder`` takes.

The reference tokenizes with transformers' ``CLIPTokenizer`` (diff-solvers-main/models/ldm/modules/encoders/modules.py:142, :151-153:
``truncation=True, max_length=77, padding="max_length"``).  This is that tokenizer written from its published rules (Radford et al. 2021,
the ``simple_tokenizer`` of the CLIP release), reading the two files every CLIP tokenizer directory holds -- ``vocab.json`` (token string ->
id) and ``merges.txt`` (one merge per line, best first, after a ``#version`` header line) -- from a LOCAL directory; nothing is loaded from
anywhere else:

  1. the text is lower-cased, whitespace runs collapse to one blank, the ends are stripped;
  2. it is split by the CLIP pattern: the two special tokens, the contractions 's 't 're 've 'm 'll 'd, runs of letters, single digits,
     runs of anything else that is not whitespace;
  3. every piece is written as UTF-8 bytes, each byte as one printable character (the byte-to-unicode table), the last one carrying
     the word-end mark ``</w>``;
  4. adjacent symbols are merged, always the pair with the best rank in ``merges.txt`` first, until no listed pair is left;
  5. ids = ``<|startoftext|>`` + symbols + ``<|endoftext|>``, truncated to 77 keeping the final ``<|endoftext|>``, padded with
     ``<|endoftext|>`` (the pad token of the SD v1 tokenizer).

Not done: the ``ftfy`` text repair and HTML un-escaping the original applies before step 1 (``ftfy`` is not a dependency of this package);
transformers falls back to a basic clean-up without it as well.  Prompts of plain text are unaffected.
"""
from __future__ import annotations

import json
import os
from functools import lru_cache
from typing import Dict, List, Sequence, Tuple

BOS, EOS = '<|startoftext|>', '<|endoftext|>'
SPLIT_PATTERN = r"<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+"


@lru_cache()
def bytes_to_unicode() -> Dict[int, str]:
    """byte -> printable character: the bytes that already print ('!'..'~', 0xA1..0xAC, 0xAE..0xFF) map to themselves, the other 68 to
    U+0100 onwards in byte order."""
    keep = list(range(ord('!'), ord('~') + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    table, n = {}, 0
    for b in range(256):
        if b in keep:
            table[b] = chr(b)
        else:
            table[b] = chr(256 + n)
            n += 1
    return table


class ClipTokenizer:
    def __init__(self, directory: str, context_length: int = 77):
        import regex
        vocab_file, merges_file = os.path.join(directory, 'vocab.json'), os.path.join(directory, 'merges.txt')
        for f in (vocab_file, merges_file):
            if not os.path.isfile(f):
                raise FileNotFoundError(f'--tokenizer_path: {f} not found (a CLIP tokenizer directory holds vocab.json and merges.txt)')
        with open(vocab_file, encoding='utf-8') as fh:
            self.encoder: Dict[str, int] = {k: int(v) for k, v in json.load(fh).items()}
        with open(merges_file, encoding='utf-8') as fh:
            lines = fh.read().split('\n')
        if lines and lines[0].startswith('#version'):
            lines = lines[1:]
        merges: List[Tuple[str, str]] = [tuple(ln.split()) for ln in lines if len(ln.split()) == 2]
        self.ranks: Dict[Tuple[str, str], int] = {m: i for i, m in enumerate(merges)}
        for t in (BOS, EOS):
            if t not in self.encoder:
                raise ValueError(f'{vocab_file} has no {t!r} entry')
        self.bos, self.eos = self.encoder[BOS], self.encoder[EOS]
        self.context_length = int(context_length)
        self.vocab_size = max(self.encoder.values()) + 1
        self._split = regex.compile(SPLIT_PATTERN, regex.IGNORECASE)
        self._cache: Dict[str, Tuple[str, ...]] = {}

    def bpe(self, piece: str) -> Tuple[str, ...]:
        """Symbols of one piece (already in byte characters) after every applicable merge, best rank first."""
        if piece in self._cache:
            return self._cache[piece]
        word = tuple(piece[:-1]) + (piece[-1] + '</w>',)
        while len(word) > 1:
            pairs = {(word[i], word[i + 1]) for i in range(len(word) - 1)}
            best = min(pairs, key=lambda p: self.ranks.get(p, float('inf')))
            if best not in self.ranks:
                break
            first, second = best
            merged, i = [], 0
            while i < len(word):
                if i + 1 < len(word) and word[i] == first and word[i + 1] == second:
                    merged.append(first + second)
                    i += 2
                else:
                    merged.append(word[i])
                    i += 1
            word = tuple(merged)
        self._cache[piece] = word
        return word

    def encode(self, text: str) -> List[int]:
        """Token ids of `text` without the start / end tokens."""
        text = ' '.join(text.split()).strip().lower()
        table = bytes_to_unicode()
        ids: List[int] = []
        for piece in self._split.findall(text):
            if piece in (BOS, EOS):
                ids.append(self.encoder[piece])
                continue
            piece = ''.join(table[b] for b in piece.encode('utf-8'))
            for sym in self.bpe(piece):
                if sym not in self.encoder:
                    raise ValueError(f'symbol {sym!r} is not in vocab.json: the vocabulary does not cover the byte alphabet')
                ids.append(self.encoder[sym])
        return ids

    def __call__(self, prompts: Sequence[str]):
        """[len(prompts), context_length] int64 tensor: start token, ids, end token; truncated keeping the end token; padded with it."""
        import torch
        if isinstance(prompts, str):
            prompts = [prompts]
        L = self.context_length
        rows = []
        for p in prompts:
            ids = [self.bos] + self.encode(p)[:L - 2] + [self.eos]
            rows.append(ids + [self.eos] * (L - len(ids)))
        return torch.tensor(rows, dtype=torch.int64).reshape(len(rows), L)
