"""The five scratch-size functions of the record side, pinned: memory use is behaviour, and each
translation unit derives its size function and its entry point's pointers from one description of
its scratch (Carver, csrc/rvz_host.hip.h), so a change to a description shows here as a moved
byte. The values were read from a build of the commit before the descriptions were unified. No
device is needed: the library loads without one."""
import pytest

N = (1, 63, 64, 65, 1025, 4097, 70001)

MERGE = {
    (8, 1): 192, (8, 63): 18368, (8, 64): 18912, (8, 65): 19504, (8, 1025): 309440,
    (8, 4097): 1237200, (8, 70001): 21069296, (6, 1): 192, (6, 63): 11424, (6, 64): 11744,
    (6, 65): 12336, (6, 1025): 194752, (6, 4097): 778448, (6, 70001): 13229296,
}   # (bs, n) at table_log2 = 0
LOSS = {
    (8, 1): 128, (8, 63): 4096, (8, 64): 4160, (8, 65): 4224, (8, 1025): 65664, (8, 4097): 262368,
    (8, 70001): 4480992, (6, 1): 128, (6, 63): 4096, (6, 64): 4160, (6, 65): 4224,
    (6, 1025): 65664, (6, 4097): 262368, (6, 70001): 4480992,
}   # (bs, n)
RECORDS = {
    (1, 1): 80, (1, 63): 2800, (1, 64): 2816, (1, 65): 2896, (1, 1025): 45136, (1, 4097): 180304,
    (1, 70001): 3080080, (63, 1): 560, (63, 63): 34064, (63, 64): 34560, (63, 65): 35120,
    (63, 1025): 553520, (63, 4097): 2212400, (63, 70001): 37800560, (64, 1): 560, (64, 63): 34544,
    (64, 64): 35072, (64, 65): 35632, (64, 1025): 561712, (64, 4097): 2245168,
    (64, 70001): 38360560, (65, 1): 592, (65, 63): 35056, (65, 64): 35584, (65, 65): 36176,
    (65, 1025): 569936, (65, 4097): 2277968, (65, 70001): 38920592, (1025, 1): 8272,
    (1025, 63): 518896, (1025, 64): 527104, (1025, 65): 535376, (1025, 1025): 8441936,
    (1025, 4097): 33742928, (1025, 70001): -1, (4097, 1): 32848, (4097, 63): 2067184,
    (4097, 64): 2099968, (4097, 65): 2132816, (4097, 1025): 33632336, (4097, 4097): 134430800,
    (4097, 70001): -1, (70001, 1): 560080, (70001, 63): 35282800, (70001, 64): 35842816,
    (70001, 65): 36402896, (70001, 1025): -1, (70001, 4097): -1, (70001, 70001): -1,
}   # (plies, n_games); -1: too many records for either board
CDF = {
    (1, 0): 64, (1, 6): 64, (1, 12): 64, (64, 0): 560, (64, 6): 560, (64, 12): 560, (65, 0): 576,
    (65, 6): 608, (65, 12): 576, (4097, 0): 32880, (4097, 6): 33904, (4097, 12): 32864,
    (2097152, 0): 16793648, (2097152, 6): 17309872, (2097152, 12): 16785456,
}   # (capacity, tile_log2)
PRIORITY = {
    0: 528, 1: 544, 32: 656, 33: 1184, 4097: 147488,
}   # nb
REFUSED = {
    "rvz_merge_scratch_size": [(7, 64, 0), (8, -1, 0), (8, 64, -1), (8, 64, 31), (8, 64, 6),
                               (8, 2 ** 31 - 1, 0)],
    "rvz_loss_scratch_size": [(7, 64), (8, -1), (8, 2 ** 31 - 1)],
    "rvz_records_scratch_size": [(0, 1), (1, 0), (-1, 4), (2 ** 31 - 1, 2), (70001, 70001)],
    "rvz_replay_cdf_size": [(0, 0), (-1, 6), (64, 5), (64, 13), (64, -1)],
    "rvz_replay_priority_scratch_size": [(-1,), (2 ** 30 + 1,)],
    "rvz_replay_is_weight_scratch_size": [(-1,)],
}


@pytest.fixture(scope="module")
def lib():
    import rvz
    return rvz.load()


def test_the_grids_are_the_ones_pinned():
    assert set(MERGE) == set(LOSS) == {(bs, n) for bs in (8, 6) for n in N}
    assert set(RECORDS) == {(p, g) for p in N for g in N}
    assert set(CDF) == {(c, t) for c in (1, 64, 65, 4097, 2 ** 21) for t in (0, 6, 12)}
    assert set(PRIORITY) == {0, 1, 32, 33, 4097}


def test_scratch_sizes_are_the_pinned_bytes(lib):
    assert {k: lib.rvz_merge_scratch_size(*k, 0) for k in MERGE} == MERGE
    assert {k: lib.rvz_loss_scratch_size(*k) for k in LOSS} == LOSS
    assert {k: lib.rvz_records_scratch_size(*k) for k in RECORDS} == RECORDS
    assert {k: lib.rvz_replay_cdf_size(*k) for k in CDF} == CDF
    assert {k: lib.rvz_replay_priority_scratch_size(k) for k in PRIORITY} == PRIORITY
    assert [lib.rvz_replay_is_weight_scratch_size(nb) for nb in (0, 1, 4097, 2 ** 30)] == [16] * 4


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_out_of_range_arguments_are_refused(lib, name):
    for args in REFUSED[name]:
        assert getattr(lib, name)(*args) == -1, args
