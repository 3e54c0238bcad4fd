"""CPU: the routing map of every configuration over a batch range, and the sweep table of the GPU batch tests against it.

A plan built on the CPU gives the kernel routing of any batch (tests/_routing.py); a boundary is a batch whose routing signature differs from
the batch before it.  tests/_routing.SWEEP must hold both sides of every boundary and every batch size real sampling runs produce
(sample.shard_seeds), so that a change that moves a threshold fails here and names the batches to add.  Building one plan on the CPU takes
4 - 60 ms (measured: CIFAR-10 ~4 ms, SD-1.5 fp16 up to ~60 ms); the whole scan is dominated by building the engines' weights."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import _routing  # noqa: E402


@pytest.fixture(scope='module')
def maps():
    return {}


def _map(maps, config):
    if config not in maps:
        maps[config] = _routing.routing_map(config)
    return maps[config]


@pytest.mark.parametrize('config', list(_routing.CONFIGS))
def test_sweep_table_holds_both_sides_of_every_routing_boundary(config, maps):
    rmap = _map(maps, config)
    table = set(_routing.SWEEP[config])
    rng = _routing.CONFIGS[config][3]
    assert table <= set(rng), sorted(table - set(rng))
    missing = []
    for b, why in _routing.boundaries(rmap):
        need = sorted({b - 1, b} - table)
        if need:
            missing.append(f'  add {need}: at B = {b} ' + ' | '.join(why))
    assert not missing, f'{config}: the sweep table lacks one side of these routing boundaries:\n' + '\n'.join(missing)


@pytest.mark.parametrize('config', list(_routing.CONFIGS))
def test_sweep_table_holds_the_ragged_batches_of_real_runs(config):
    net, _, _, rng, bench = _routing.CONFIGS[config]
    ragged = [b for b in _routing.ragged_batches(net) if b in rng]
    assert bench in _routing.SWEEP[config]
    missing = sorted(set(ragged) - set(_routing.SWEEP[config]))
    assert not missing, f'{config}: add the batch sizes sample.shard_seeds hands a rank: {missing}'


def test_ragged_batches_come_from_the_reference_partition():
    """The batches of the issue's table, as sample.shard_seeds computes them (not typed by hand into the sweep)."""
    assert {255, 256} <= set(_routing.ragged_batches('cifar10')) and {63, 64, 127, 128} <= set(_routing.ragged_batches('cifar10'))
    assert {63, 64, 127, 128} <= set(_routing.ragged_batches('ffhq'))
    assert {63, 64} <= set(_routing.ragged_batches('imagenet64'))
    assert 15 in _routing.ragged_batches('sd15')


def test_the_routing_thresholds_the_documents_state(maps):
    """the fp32 attention's channel-split block below 128 images (16x16 attention of CIFAR-10 / FFHQ-64); the 256-pixel
    tiles of the CIFAR-10 16x16 layers from 256 images; the <= 4-row projection kernel (2573) up to 4 embedding rows."""
    for config in ('cifar10_fp32', 'ffhq_fp32'):
        rmap = _map(maps, config)
        why = dict(_routing.boundaries(rmap))
        assert 128 in why and 'attention channel_split -> query_split' in ' '.join(why[128])
        assert 5 in why and 'kernel 2573 -> 0' in ' '.join(why[5])
    why = dict(_routing.boundaries(_map(maps, 'cifar10_fp32')))
    assert 256 in why and 'kernel 128 -> 2565' in ' '.join(why[256])


def test_sd15_fp16_routes_the_f16_oracle_layer_set_at_every_swept_batch():
    """The SD-1.5 fp16 sweep checks its golden slots against the fp16-operand oracle (tests/golden/ldm_sd15_f16ops.npz), which is valid only
    where the plan rounds exactly the oracle's layers: at every batch of the table, both sigma forms."""
    import numpy as np
    from _f16_names import ldm_prefixes
    want = [str(v) for v in np.load(os.path.join(ROOT, 'tests', 'golden', 'ldm_sd15_f16ops.npz'))['f16_layers']]
    eng = _routing.make_engine('sd15_fp16')
    for B in _routing.SWEEP['sd15_fp16']:
        for rows in _routing.sigma_forms('sd15_fp16', B):
            assert sorted(ldm_prefixes(_routing.plan_of(eng, 'sd15_fp16', B, rows))) == want, (B, rows)
            eng._plans.clear()


def test_cli_batch_sizes_of_the_byte_identity_test_route_every_row_identically():
    """tests/test_hip_sample_cli.py compares PNG bytes of `--batch 5` and `--batch 3` runs over 13 seeds on tiny_song: shard_seeds makes
    batches of 5 / 4 / 4 and 3 / 3 / 3 / 2 / 2 images.  The samplers evaluate at one host-float sigma per step (shared sigma: one embedding
    row), and at that form every one of those batch sizes routes every launch identically -- so the byte-for-byte assertion holds by
    construction, not by luck of rounding.  (With per-sample sigma the embedding projections would leave the <= 4-row kernel at 5.)"""
    from diff_sampler_amd import sample
    seeds = list(range(12)) + [1003]
    sizes = sorted({len(b) for mb in (5, 3) for b in sample.shard_seeds(seeds, mb, 0, 1)})
    assert sizes == [2, 3, 4, 5]
    rmap = _routing.routing_map('tiny_song', batches=sizes)
    shared = {B: dict(rmap[B])['shared sigma'] for B in sizes}
    assert all(shared[B] == shared[sizes[0]] for B in sizes), [(B, _routing.diff(list(shared[sizes[0]]), list(shared[B]))) for B in sizes]


@pytest.mark.parametrize('config', [c for c in _routing.CONFIGS if len(_routing.sigma_forms(c, 2)) == 2])
def test_shared_sigma_form_adds_no_boundary_of_its_own(config, maps):
    """The GPU sweep evaluates the per-sample sigma form at every swept batch (the samplers run the shared form at the ragged batches): that
    covers every routing only while each boundary of the shared-sigma plans is also a boundary of the per-sample plans."""
    rmap = _map(maps, config)
    per_sample = {B: dict(v)['per-sample sigma'] for B, v in rmap.items()}
    shared = {B: dict(v)['shared sigma'] for B, v in rmap.items()}
    only_shared = [(B, _routing.diff(list(shared[B - 1]), list(shared[B])))
                   for B in sorted(rmap)[1:] if shared[B] != shared[B - 1] and per_sample[B] == per_sample[B - 1]]
    assert not only_shared, f'{config}: boundaries of the shared-sigma form alone (the GPU sweep does not run that form): {only_shared}'
