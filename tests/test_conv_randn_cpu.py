"""CPU-only: the shared pieces of the convolution kernels' randn comparison (tests/_conv_randn.py).  The Winograd case table still makes
the inputs it made when its five groups were five test files, bit for bit; and the one checker, fed an fp32 rounding of the reference,
passes -- and fails on each kind of damage one of the five copies used to catch."""
import hashlib
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _conv_randn as R  # noqa: E402

GROUPS = R.wino_groups(256)
INPUTS_SHA256 = '63f9c649ab6bf1253012ddfea9f9d15b8c6b6914b36beb232c576fc8fa92213c'      # from the five files, at 256 compute units
GUARD = 8


def test_case_table_keeps_its_cases_and_their_input_bits():
    assert list(GROUPS) == ['pipe', 'base', 'pipe2', 'kloop', 'persist']
    assert [len(t) for t in GROUPS.values()] == [10, 4, 7, 12, 7]
    names = [n for t in GROUPS.values() for n in t]
    assert len(names) == 40 and len(set(names)) == 40
    assert set(GROUPS['persist']) == set(R.PERSIST_TILES)
    total = hashlib.sha256()
    for table in GROUPS.values():
        for row in table.values():
            d, h = R.make_layer(*row), hashlib.sha256()
            for k in sorted(d):
                if k != 'ref' and d[k] is not None:        # the fp64 reference's bits may depend on the CPU's thread count
                    h.update(k.encode())
                    h.update(d[k].contiguous().numpy().tobytes())
            total.update(h.digest())
    assert total.hexdigest() == INPUTS_SHA256


def test_persist_group_has_the_tile_counts_it_is_named_after():
    for name, row in GROUPS['persist'].items():
        counts, padded = R.tiles_per_workgroup(row[1], row[2], row[5], 256)
        assert (max(counts), min(counts)) == R.PERSIST_TILES[name], name


def _perfect(row):
    """What a faultless kernel would hand to compare(): the fp32 rounding of the reference and its column sums over consecutive 64-row
    blocks, inside NaN-margined buffers."""
    B, H, cout = row[1], row[2], row[5]
    got = R.make_layer(*row)['ref'].float()
    blocks = got.double().reshape(B * H * H // 64, 64, cout)
    stats = torch.stack([blocks.sum(1), (blocks ** 2).sum(1)], 1).float().reshape(-1)
    bufs = [torch.cat([torch.full((GUARD,), float('nan')), t.reshape(-1), torch.full((GUARD,), float('nan'))]) for t in (got, stats)]
    return got, stats, bufs[0], bufs[1]


ONE, TWO = GROUPS['pipe']['one_slab'], GROUPS['pipe']['two_slabs']          # one image and two images of 16 x 16


@pytest.mark.parametrize('row', [ONE, TWO], ids=['one_image', 'two_images'])
def test_checker_passes_the_rounded_reference_and_fails_each_kind_of_damage(row):
    B, hw, cout = row[1], row[2] * row[2], row[5]
    err, per, e_s, e_q = R.compare(row, *_perfect(row))
    print(f'fp32 rounding of the reference: rel err {err:.3e}, column sums {e_s:.3e} / {e_q:.3e}')
    assert len(per) == B

    def fails(damage, match=None):
        got, stats, out_buf, stats_buf = _perfect(row)
        damage(got, stats, out_buf, stats_buf)
        with pytest.raises(AssertionError, match=match):
            R.compare(row, got, stats, out_buf, stats_buf)

    def move_one_element(got, stats, out_buf, stats_buf):
        got[hw - 3, 5] += 1e-4 * float(R.make_layer(*row)['ref'].abs().max())

    def nan_in_output(got, stats, out_buf, stats_buf):
        got[hw - 3, 5] = float('nan')

    fails(move_one_element)
    fails(nan_in_output)
    for which, at in ((2, 0), (2, -1), (3, 0), (3, -1)):        # out_buf / stats_buf, front / back margin
        fails(lambda *t: t[which].__setitem__(at, 1.0))
    if B == 2:
        def swap_images(got, stats, out_buf, stats_buf):
            got.copy_(got.reshape(2, hw, cout).flip(0).reshape(-1, cout))

        def move_a_statistics_block_to_the_other_image(got, stats, out_buf, stats_buf):
            st = stats.view(2, hw // 64, 2 * cout)
            st[0, 0], st[1, 0] = st[1, 0].clone(), st[0, 0].clone()

        fails(swap_images)
        fails(move_a_statistics_block_to_the_other_image)
