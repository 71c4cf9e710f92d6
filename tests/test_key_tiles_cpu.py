"""The host-side key-tile table of the frozen layers (ops.key_tile_table, host_metadata) against a brute-force loop."""
import torch


def _brute(mask):
    B, T = mask.shape
    table, n = [[-1] * (T // 64) for _ in range(B)], 0
    for b in range(B):
        for j in range(T // 64):
            if any(int(mask[b, s]) != 0 for s in range(64 * j, 64 * j + 64)):
                table[b][j] = n
                n += 1
    return torch.tensor(table, dtype=torch.int32), 64 * n


def _masks():
    T = 256
    m = torch.zeros(6, T, dtype=torch.long)
    m[0] = 1                                   # no pad
    m[1, :64] = 1                              # a prompt of exactly 64 keys
    m[2, :70] = 1; m[2, 192:202] = 1           # tile 2 dead, tiles 1 and 3 partly live
    m[3, :64] = 1; m[3, 192] = 1               # one valid key in the last tile
    m[4, :1] = 1                               # a single key
    m[5, 63] = 1; m[5, 64] = 1                 # the last key of one tile and the first of the next
    return m


def test_key_tile_table_matches_brute_force():
    from mmgl_amd import ops
    m = _masks()
    table, m_live = ops.key_tile_table(m)
    want, want_live = _brute(m)
    assert table.dtype == torch.int32 and table.shape == (6, 4)
    assert torch.equal(table, want) and m_live == want_live
    assert table[0].tolist() == [0, 1, 2, 3] and table[1].tolist() == [4, -1, -1, -1] and table[2].tolist() == [5, 6, -1, 7]
    g = torch.Generator().manual_seed(3)
    r = (torch.rand(5, 640, generator=g) < 0.004).long()          # sparse random masks: many dead tiles, some empty samples
    table, m_live = ops.key_tile_table(r)
    want, want_live = _brute(r)
    assert torch.equal(table, want) and m_live == want_live
    assert ops.key_tile_table(torch.ones(2, 100, dtype=torch.long)) == (None, 0)      # T is no multiple of 64: no table
    assert ops.key_tile_table(torch.zeros(2, 128, dtype=torch.long))[1] == 0


def test_host_metadata_carries_the_table():
    from mmgl_amd.model.modelling_cross_attention import host_metadata
    m = _masks()
    meta = host_metadata({"attention_mask": m})
    want, want_live = _brute(m)
    assert torch.equal(meta["key_tiles"], want) and meta["M_live"] == want_live
    meta = host_metadata({"attention_mask": torch.ones(2, 100, dtype=torch.long)})
    assert "key_tiles" not in meta and "M_live" not in meta
