"""A small CLIP-format tokenizer directory written by the tests (tests/test_clip_cpu.py, tests/test_hip_text_encoder.py)."""
import json
import os


def write_tokenizer(directory, merges=(('l', 'o'), ('lo', 'w</w>'), ('e', 'r</w>'), ('n', 'e'), ('ne', 'w'), ('h', 'i</w>'))):
    """A small CLIP-format tokenizer directory: the 256 byte characters, their word-end forms, the merged symbols in merge order, the two
    special tokens last (the layout of the released vocabulary).  Returns the vocabulary."""
    from diff_sampler_amd.clip_tokenizer import bytes_to_unicode
    chars = [bytes_to_unicode()[b] for b in range(256)]
    syms = chars + [c + '</w>' for c in chars] + [a + b for a, b in merges] + ['<|startoftext|>', '<|endoftext|>']
    vocab = {s: i for i, s in enumerate(syms)}
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, 'vocab.json'), 'w', encoding='utf-8') as fh:
        json.dump(vocab, fh)
    with open(os.path.join(directory, 'merges.txt'), 'w', encoding='utf-8') as fh:
        fh.write('#version: 0.2\n' + '\n'.join(f'{a} {b}' for a, b in merges) + '\n')
    return vocab
