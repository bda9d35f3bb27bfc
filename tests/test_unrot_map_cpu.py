"""CPU: the index map of the fused un-rotation kernels (tests/unrot_model.py) against the oracle's Shift2d + rotate
(oracle/networks.py: shift_down, rot90cw) at P = 64, all four rotations: the gather of the backward kernel, the dropped
and the zero row, and how a 2x2 output tile of the stack lies in the un-rotated plane."""
import numpy as np
import pytest
import torch

from unrot_model import unrot_map, zero_line

P = 64
ANGLES = (0, 270, 180, 90)


def _oracle_plane(k):
    """f's plane for the stack plane d[s, v] = 1 + s * P + v (0 marks what no stack element reaches)."""
    from oracle.networks import rot90cw, shift_down
    d = (1 + torch.arange(P * P, dtype=torch.float64)).reshape(1, 1, P, P)
    return rot90cw(shift_down(d), ANGLES[k])[0, 0].numpy()


@pytest.mark.parametrize("k", range(4))
def test_map_is_the_oracles_shift_and_rotation(k):
    f = _oracle_plane(k)
    i, j, kept = unrot_map(k, P)
    d = 1 + np.arange(P * P, dtype=np.float64).reshape(P, P)
    assert kept[:P - 1].all() and not kept[P - 1].any()
    assert i[kept].min() >= 0 and i[kept].max() < P and j[kept].min() >= 0 and j[kept].max() < P
    assert np.array_equal(f[i[kept], j[kept]], d[kept])                   # forward store / backward gather address
    z = zero_line(k, P)
    assert z.sum() == P and np.array_equal(f == 0, z)                      # the zero row, and nothing else, is unreached
    want = {0: z[0, :].all(), 1: z[:, P - 1].all(), 2: z[P - 1, :].all(), 3: z[:, 0].all()}[k]
    assert want
    # backward: gd = gather of gf through the map, +0 on the dropped row == the vjp of the oracle's forward
    from oracle.networks import rot90cw, shift_down
    x = torch.arange(P * P, dtype=torch.float64).reshape(1, 1, P, P).requires_grad_(True)
    gf = torch.randn(1, 1, P, P, dtype=torch.float64, generator=torch.Generator().manual_seed(k))
    rot90cw(shift_down(x), ANGLES[k]).backward(gf)
    gd = np.zeros((P, P))
    gd[kept] = gf[0, 0].numpy()[i[kept], j[kept]]
    assert np.array_equal(gd, x.grad[0, 0].numpy()) and not np.signbit(gd[P - 1]).any()


@pytest.mark.parametrize("k", range(4))
def test_a_2x2_tile_stays_a_2x2_block(k):
    """Output tile (rows 2ty, 2ty+1; columns 2tx, 2tx+1) of the stack, values o0[0], o0[1] / o1[0], o1[1]: under 0 and
    180 degrees the horizontally adjacent pair in f is (o0[0], o0[1]) (reversed for 180), under 90 and 270 degrees it
    is (o0[c], o1[c]); after the one-row shift the pairs of 0 / 180 start on even columns (8-byte aligned), those of
    90 / 270 on odd ones."""
    i, j, kept = unrot_map(k, P)
    for ty in range(P // 2):
        for tx in (0, 1, P // 2 - 1):
            r, c = 2 * ty, 2 * tx
            if k in (0, 2):
                for row in (r, r + 1):
                    if not kept[row, c]:
                        continue
                    assert i[row, c] == i[row, c + 1] and abs(j[row, c] - j[row, c + 1]) == 1
                    assert (j[row, c + 1] - j[row, c]) == (1 if k == 0 else -1)
                    assert min(j[row, c], j[row, c + 1]) % 2 == 0
            elif kept[r + 1, c]:
                for col in (c, c + 1):
                    assert i[r, col] == i[r + 1, col] and abs(j[r, col] - j[r + 1, col]) == 1
                    assert min(j[r, col], j[r + 1, col]) % 2 == 1
            else:       # the tile's second row is the dropped one: single elements
                assert kept[r, c] and not kept[r + 1, c]


@pytest.mark.parametrize("k", range(4))
def test_tile_stores_write_every_element_of_the_plane_once(k):
    """The store list of the Winograd output transform (unrot_model.tile_stores), over all 32 x 32 tiles of a plane:
    every element of f's plane is written exactly once, with the oracle's value (0 on the zero line); 8-byte stores of
    0 / 180 degrees are 8-byte aligned, those of 90 / 270 degrees only 4-byte aligned."""
    from unrot_model import tile_stores
    f = _oracle_plane(k)
    d = 1 + np.arange(P * P, dtype=np.float64).reshape(P, P)
    got = np.full(P * P, np.nan)
    for s0 in range(0, P, 2):
        for v0 in range(0, P, 2):
            for off, vals in tile_stores(k, P, s0, v0):
                assert 0 <= off and off + len(vals) <= P * P and off // P == (off + len(vals) - 1) // P   # one row
                if len(vals) == 2:
                    assert off % 2 == (0 if k in (0, 2) else 1)
                for q, v in enumerate(vals):
                    assert np.isnan(got[off + q]), "written twice"
                    got[off + q] = 0.0 if v == 0 else d[s0 + v[1], v0 + v[2]]
    assert np.array_equal(got.reshape(P, P), f)
