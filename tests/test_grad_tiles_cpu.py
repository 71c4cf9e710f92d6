"""The host side of the live-first gradient rows: the destination table and row map (ops.grad_tile_table, KeyTiles.dest / grad_rows)
against a brute-force loop, and the static schedule of mmgl_gemm_nt_rowk (mmgl_gemm_nt_rowk_item: the function the kernel itself
evaluates) against its balance bound."""
import pytest
import torch

from test_key_tiles_cpu import _masks


def _brute(mask):
    """(dest [B, T // 64], rows [B * T], m_live): live tiles in order first, the dead tiles in order behind them."""
    B, T = mask.shape
    nt = T // 64
    live = [[any(int(mask[b, s]) != 0 for s in range(64 * j, 64 * j + 64)) for j in range(nt)] for b in range(B)]
    n_live = sum(sum(r) for r in live)
    dest, nl, nd = [[0] * nt for _ in range(B)], 0, 0
    for b in range(B):
        for j in range(nt):
            if live[b][j]:
                dest[b][j], nl = nl, nl + 1
            else:
                dest[b][j], nd = n_live + nd, nd + 1
    rows = [64 * dest[b][t // 64] + t % 64 for b in range(B) for t in range(T)]
    return torch.tensor(dest, dtype=torch.int32), torch.tensor(rows, dtype=torch.int32), 64 * n_live


def _cases():
    g = torch.Generator().manual_seed(11)
    return [_masks(), (torch.rand(5, 640, generator=g) < 0.004).long(), (torch.rand(7, 320, generator=g) < 0.01).long(),
            torch.ones(2, 128, dtype=torch.long)]


@pytest.mark.parametrize("i", range(4))
def test_destination_table_and_row_map_match_brute_force(i):
    from mmgl_amd import ops
    m = _cases()[i]
    table, m_live = ops.key_tile_table(m)
    want_dest, want_rows, want_live = _brute(m)
    assert m_live == want_live
    kt = ops.KeyTiles(table, m_live, "cpu")
    assert kt.dest.dtype == torch.int32 and kt.grad_rows.dtype == torch.int32
    assert torch.equal(kt.dest, want_dest) and torch.equal(kt.grad_rows, want_rows)
    # a permutation of the tiles: live tiles keep their compact index, the dead ones follow in order
    flat, t = kt.dest.reshape(-1), table.reshape(-1)
    assert sorted(flat.tolist()) == list(range(flat.numel()))
    assert torch.equal(flat[t >= 0], t[t >= 0]) and flat[t < 0].tolist() == list(range(m_live // 64, flat.numel()))
    assert sorted(kt.grad_rows.tolist()) == list(range(m.numel()))
    assert torch.equal(kt.grad_rows[kt.rowmap >= 0], kt.rowmap[kt.rowmap >= 0])       # a live row goes where the compact copy has it


def _schedule(G, n_long, n_short, q):
    from mmgl_amd import _lib
    item = _lib.lib().mmgl_gemm_nt_rowk_item
    per_wg = []
    for wg in range(G):
        mine, it = [], 0
        while (v := item(G, n_long, n_short, q, wg, it)) >= 0:
            mine.append(v)
            it += 1
        assert item(G, n_long, n_short, q, wg, it + 1) < 0           # nothing behind the first gap
        per_wg.append(mine)
    return per_wg


@pytest.mark.parametrize("G,n_long,n_short,q", [(256, 776, 504, 3), (256, 0, 1280, 3), (256, 1280, 0, 3), (256, 0, 37, 3), (256, 300, 0, 3),
                                                (10, 3, 4, 3), (7, 5, 1, 3), (256, 8, 1272, 3), (256, 255, 1025, 3), (256, 776, 504, 1),
                                                (16, 48, 112, 3), (256, 1, 2000, 24)])
def test_rowk_schedule_hands_out_every_tile_once_and_balanced(G, n_long, n_short, q):
    """Every tile exactly once; a workgroup's long tiles come before its short ones; with a long tile weighing q short ones, no
    workgroup carries more than ceil(total / G) plus one long tile.  (776, 504) on 256 workgroups is the bench batch's fused dgrad:
    12 units, against 14 for plain round-robin over 'long tiles first'."""
    grid = min(G, n_long + n_short)
    per_wg = _schedule(grid, n_long, n_short, q)
    flat = sorted(v for mine in per_wg for v in mine)
    assert flat == list(range(n_long + n_short))
    total = q * n_long + n_short
    loads = []
    for mine in per_wg:
        kinds = [v < n_long for v in mine]
        assert kinds == sorted(kinds, reverse=True)
        loads.append(sum(q if k else 1 for k in kinds))
    assert max(loads) <= -(-total // grid) + q
    assert all(mine for mine in per_wg)                               # the grid is min(CUs, tiles): nobody starts without an item
    if (G, n_long, n_short, q) == (256, 776, 504, 3):
        assert max(loads) == 12 and min(loads) == 11
    if n_long == 0 or n_short == 0:                                   # one class: the plain round-robin of the persistent kernel
        assert all(mine == list(range(wg, n_long + n_short, grid)) for wg, mine in enumerate(per_wg))


def test_rowk_item_rejects_bad_arguments():
    from mmgl_amd import _lib
    item = _lib.lib().mmgl_gemm_nt_rowk_item
    assert item(0, 1, 1, 3, 0, 0) == -1 and item(4, 1, 1, 0, 0, 0) == -1 and item(4, 1, 1, 3, 4, 0) == -1 and item(4, -1, 1, 3, 0, 0) == -1
