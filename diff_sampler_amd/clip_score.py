"""CLIP score on the engine: the reference's ``clip_score.py`` (the same file in diff-solvers-main, gits-main, amed-solver-main, sfd-main).

    python -m diff_sampler_amd.clip_score calc --images DIR --prompts captions.csv --model CKPT --tokenizer_path DIR

Per batch the reference preprocesses every image on the host through open_clip's transform (clip_score.py:81), tokenizes the captions (:82),
runs both towers (:84-85), normalises the features (:86-87) and sums ``100 * <image, text>`` (:89-90); the average over the images is the
score (:93-94).  Here: ``preprocess`` is that transform up to the uint8 image (RGB, PIL bicubic resize of the shorter side, centre crop --
mean / std are applied on the device), ``clip_score_engine`` runs the towers on engine kernels, ``dsm_clip_score`` (csrc/metrics/clip_score.hip)
is the normalise-multiply-sum with the per-pair values in fp32 as the reference has them and their sum in fp64.

The CLIP weights are a local file (``--model``: a HF ``CLIPModel`` or an open_clip state dict, ``.pt`` / ``.bin`` / ``.pth``; nothing is
downloaded), the captions a csv with a ``text`` column (``--prompts``; the reference fetches the COCO captions file itself), the tokenizer
a directory holding ``vocab.json`` and ``merges.txt`` (``clip_tokenizer``).

``--dtype fp16x3`` (``ClipScorer(..., dtype='fp16x3')``): the four projections of every transformer layer run as split-fp16 GEMMs with fp32
operands and results (``dsm_gemm_split``, csrc/metrics/gemm_split.hip) -- fp32 tolerances at about 2.3 times the tower throughput.  The
activations entering a projection must stay within fp16's range (65504); the scorer checks the features of every batch and raises otherwise.

CAPTION PAIRING: image i of the sorted FULL listing goes with caption i.  That equals the reference whenever no subset is taken.  With
``--num`` the reference pairs position j of the shuffled-and-sorted subset with caption j (clip_score.py:79 slices the captions by subset
position while dataset.py picked other images), i.e. it scores images against other images' captions; that is not reproduced.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _metrics_lib, clip_score_arch as arch
from .fid import ImageFolder, _init_dist, shard_items


# ---- host preprocessing -------------------------------------------------------------------------------------------------------------------
def preprocess(image, size: int = 224) -> torch.Tensor:
    """PIL image -> uint8 [3, size, size]: open_clip's inference transform without its float stages -- RGB, bicubic (PIL's own, antialiased)
    resize of the shorter side to `size` with the longer side ``int(size * long / short)``, centre crop at ``int(round((h - size) / 2))``."""
    import PIL.Image
    image = image.convert('RGB')
    w, h = image.size
    if (w, h) != (size, size):
        if w <= h:
            nw, nh = size, int(size * h / w)
        else:
            nw, nh = int(size * w / h), size
        if (nw, nh) != (w, h):
            image = image.resize((nw, nh), PIL.Image.BICUBIC)
        top, left = int(round((nh - size) / 2.0)), int(round((nw - size) / 2.0))
        image = image.crop((left, top, left + size, top + size))
    a = np.asarray(image, dtype=np.uint8)
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))


def read_captions(path):
    """The ``text`` column of a csv (clip_score.py:50-55)."""
    import csv
    with open(path, 'r', newline='', encoding='utf-8') as fh:
        reader = csv.DictReader(fh)
        if 'text' not in (reader.fieldnames or ()):
            raise ValueError(f'{path}: no "text" column (found {reader.fieldnames})')
        return [row['text'] for row in reader]


def pair_captions(dataset_idx, captions):
    """Caption of every image of a (possibly subsampled) listing: image i of the sorted full listing goes with caption i."""
    idx = [int(i) for i in dataset_idx]
    if idx and max(idx) >= len(captions):
        raise ValueError(f'{len(captions)} captions for an image listing that reaches index {max(idx)}')
    return [captions[i] for i in idx]


def result_line(image_path, avg, desc=None):
    """The line sfd-main/clip_score.py:97-100 appends to clip_score.txt: ``<desc> <score>``, or the last two path components and the score."""
    if desc is not None:
        return f'{desc} {avg}\n'
    parts = ([''] + str(image_path).split('/'))[-2:]
    return f'{parts[0]} {parts[1]} {avg}\n'


def load_state_dict(path):
    """A HF or open_clip state dict from ``.pt`` / ``.bin`` / ``.pth`` (tensors only; a ``state_dict`` wrapper key is unwrapped)."""
    if not str(path).endswith(('.pt', '.bin', '.pth')):
        raise ValueError(f'--model: {path} is not a .pt / .bin / .pth state dict')
    sd = torch.load(path, map_location='cpu', weights_only=True)
    if isinstance(sd, dict) and 'state_dict' in sd and isinstance(sd['state_dict'], dict):
        sd = sd['state_dict']
    return sd


# ---- the scorer ---------------------------------------------------------------------------------------------------------------------------
class ClipScorer:
    """``ClipScorer(spec, params, tokenizer).score(images_u8, tokens_or_prompts) -> [B]`` fp32: ``100 * cos(image feature, text feature)``."""

    def __init__(self, spec: arch.ClipScoreSpec, params, tokenizer=None, device='cuda', dtype='fp32'):
        from .clip_score_engine import ClipImageEncoder, ClipPooledTextEncoder
        self.spec, self.tokenizer, self.device, self.dtype = spec, tokenizer, torch.device(device), dtype
        self.image = ClipImageEncoder(spec, params, device, dtype=dtype)
        self.text = ClipPooledTextEncoder(spec, params, device, dtype=dtype)
        self.mlib = _metrics_lib.load()
        self.total = torch.zeros(1, dtype=torch.float64, device=self.device)       # running fp64 sum of every score() since reset()

    @classmethod
    def from_config(cls, name='vit_g_14', seed=0, **kw):
        spec = arch.named_spec(name)
        return cls(spec, arch.init_clip_score_params(spec, seed), **kw)

    @classmethod
    def from_checkpoint(cls, path, tokenizer=None, device='cuda', act='gelu', dtype='fp32'):
        sd = load_state_dict(path)
        spec = arch.spec_from_state_dict(sd, act=act)
        params = arch.from_open_clip(spec, sd) if arch.is_open_clip(sd) else arch.params_from_state_dict(spec, sd)
        return cls(spec, params, tokenizer, device, dtype=dtype)

    def tokens(self, tokens_or_prompts) -> torch.Tensor:
        x = tokens_or_prompts
        if isinstance(x, str) or (isinstance(x, (list, tuple)) and x and isinstance(x[0], str)):
            if self.tokenizer is None:
                raise ValueError('prompts given as text need a tokenizer (ClipScorer(..., tokenizer=ClipTokenizer(directory)))')
            return self.tokenizer(x)
        return torch.as_tensor(x)

    def reset(self):
        self.total.zero_()

    def score(self, images_u8, tokens_or_prompts) -> torch.Tensor:
        from . import _lib
        t = self.tokens(tokens_or_prompts)
        if t.shape[0] != len(images_u8):
            raise ValueError(f'{len(images_u8)} images for {t.shape[0]} prompts')
        fi, _ = self.image.raw(images_u8)
        ft, _ = self.text.raw(t)
        B, E = fi.shape
        if self.dtype == 'fp16x3':
            for which, f in (('image', fi), ('text', ft)):
                if not bool(torch.isfinite(f).all()):
                    raise FloatingPointError(f"{which} features are not finite: dtype='fp16x3' splits every projection input into fp16 halves and "
                                             f'holds activations up to 65504 in magnitude only; score this model with --dtype fp32')
        scores = torch.empty(B, dtype=torch.float32, device=self.device)
        vp = lambda x: C.c_void_p(x.data_ptr())
        _metrics_lib.check(self.mlib.dsm_clip_score(vp(fi), E, vp(ft), E, B, E, vp(scores), vp(self.total), _lib.stream_ptr()), 'dsm_clip_score')
        return scores

    def score_raw(self, images_hwc_u8, tokens_or_prompts) -> torch.Tensor:
        """``score`` of undecorated images: uint8 [B, H, W, 3] of one size, host or device; the resize of the shorter side to the tower's
        input size and the centre crop run on the device (clip_preprocess: the bits of ``preprocess``)."""
        from .clip_preprocess import resize_center_crop
        return self.score(resize_center_crop(images_hwc_u8, self.spec.image_size, self.device), tokens_or_prompts)


def resize_mixed(arrays, size, device) -> torch.Tensor:
    """Decoded RGB arrays [h, w, 3] of any mix of sizes -> device uint8 [B, 3, size, size] in the arrays' order: one device resize per
    size (groups in order of first appearance)."""
    from . import clip_preprocess
    groups = {}
    for j, a in enumerate(arrays):
        groups.setdefault(tuple(a.shape[:2]), []).append(j)
    out = None
    for members in groups.values():
        x = clip_preprocess.resize_center_crop(torch.from_numpy(np.stack([arrays[j] for j in members])), size, device)
        if len(groups) == 1:
            return x
        if out is None:
            out = torch.empty(len(arrays), *x.shape[1:], dtype=x.dtype, device=x.device)
        out[torch.as_tensor(members, device=x.device)] = x
    return out


# ---- command line -------------------------------------------------------------------------------------------------------------------------
def calc_clip_score(scorer, image_path, captions, num_expected=None, seed=0, max_batch_size=64, log=print, device_resize=False):
    """clip_score.py:43-94 with the model injected: list, shard over ranks, score, SUM-all-reduce, average.  Returns (average, images).
    `device_resize`: PIL only decodes (``convert('RGB')``); the images of a batch are grouped by size and every group is resized,
    cropped on the device; the batch is scored in one call as on the host path, so the scores and the total have the host path's bits."""
    import torch.distributed as dist
    ds = ImageFolder(image_path, max_size=num_expected, random_seed=seed)
    if num_expected is not None and len(ds) < num_expected:
        raise ValueError(f'Found {len(ds)} images, but expected at least {num_expected}')
    if len(ds) < 1:
        raise ValueError(f'Found no images under {image_path}')
    texts = pair_captions(ds.idx, captions)
    rank, world = (dist.get_rank(), dist.get_world_size()) if (dist.is_available() and dist.is_initialized()) else (0, 1)
    log(f'Calculating statistics for {len(ds)} images...')
    import PIL.Image
    scorer.reset()
    size = scorer.spec.image_size
    for idx in shard_items(len(ds), max_batch_size, rank, world):
        if world > 1:
            dist.barrier()
        if len(idx) == 0:
            continue
        files = [os.path.join(ds.path, ds.names[int(ds.idx[i])]) for i in idx.tolist()]
        if device_resize:
            imgs = resize_mixed([np.asarray(PIL.Image.open(f).convert('RGB'), dtype=np.uint8) for f in files], size, scorer.device)
        else:
            imgs = torch.stack([preprocess(PIL.Image.open(f), size) for f in files])
        scorer.score(imgs, [texts[i] for i in idx.tolist()])
    total = scorer.total.clone()
    if world > 1:
        dist.all_reduce(total)
    return float(total.item()) / len(ds), len(ds)


try:
    import click
except ImportError:                        # pragma: no cover
    click = None

if click is not None:
    @click.group()
    def main():
        """Calculate CLIP score -- the reference's clip_score.py surface with the model, captions and tokenizer as local files."""

    @main.command()
    @click.option('--images', 'image_path', help='Path to the images', metavar='PATH', type=str, required=True)
    @click.option('--prompts', 'prompt_path', help='csv with a "text" column: caption i belongs to image i of the sorted listing', type=str, required=True)
    @click.option('--model', 'model_path', help='CLIP state dict (HF CLIPModel or open_clip layout): .pt / .bin / .pth', type=str, required=True)
    @click.option('--tokenizer_path', help='Directory with vocab.json and merges.txt', type=str, required=True)
    @click.option('--num', 'num_expected', help='Number of images to use', metavar='INT', type=click.IntRange(min=2), show_default=True)
    @click.option('--seed', help='Random seed for selecting the images', metavar='INT', type=int, default=0, show_default=True)
    @click.option('--batch', help='Maximum batch size', metavar='INT', type=click.IntRange(min=1), default=64, show_default=True)
    @click.option('--desc', help='A description string (written to clip_score.txt in place of the folder names)', metavar='str', type=str)
    @click.option('--device', type=str, default=None)
    @click.option('--device_resize', help='Resize and crop on the device (the same bits as the host transform)', is_flag=True)
    @click.option('--dtype', help='fp16x3: the towers\' projections on the fp16 matrix pipe with split fp32 operands (fp32 accuracy, activations up to 65504)',
                  type=click.Choice(['fp32', 'fp16x3']), default='fp32', show_default=True)
    def calc(image_path, prompt_path, model_path, tokenizer_path, num_expected, seed, batch, desc, device, device_resize, dtype):
        """Calculate the CLIP score of a folder of images against their captions."""
        from .clip_tokenizer import ClipTokenizer
        dist, rank = _init_dist()
        device = device or ('cuda:%d' % int(os.environ.get('LOCAL_RANK', 0)))
        log = print if rank == 0 else (lambda *a, **k: None)
        log(f'Loading images from "{image_path}"...')
        captions = read_captions(prompt_path)
        log(f'Loading the CLIP model from "{model_path}"...')
        with torch.no_grad():
            scorer = ClipScorer.from_checkpoint(model_path, ClipTokenizer(tokenizer_path), device, dtype=dtype)
            avg, n = calc_clip_score(scorer, image_path, captions, num_expected=num_expected, seed=seed, max_batch_size=batch, log=log,
                                     device_resize=device_resize)
        if rank == 0:
            print(f'CLIP score: {avg}')
            with open('clip_score.txt', 'a') as fh:
                fh.write(result_line(image_path, avg, desc))
        if dist.is_initialized():
            dist.barrier()

    if __name__ == '__main__':
        main()
