"""The argument checks of the stateless entry points (include/rvz.h), which run before any HIP
call and so need no GPU: every function that takes a board size refuses a size that is neither 8
nor 6, a negative row count and a null required pointer, and answers n = 0 with null pointers
without a launch. The expected codes are the library's recorded answers, per function, from before
the host layer's launch path was shared (csrc/rvz_host.hip.h): rvz_alphabeta reads its weights on
the host whatever n is, so a null there is RVZ_EINVAL at n = 0 too.

No call here may launch: a call that passes its checks returns before HIP (n = 0), and every
other one is refused. Where a HIP device is present the non-null pointers are real device
memory all the same, so a check that went missing would fail this test and nothing else."""
import ctypes as C

import pytest
import torch

OK, EINVAL = 0, -22
SLOT = 1 << 16          # bytes between two pointer arguments of one call


@pytest.fixture(scope="module")
def lib():
    import rvz
    return rvz.load()


@pytest.fixture(scope="module")
def pointers():
    """16 distinct 16-byte aligned non-null addresses: device memory when there is a device,
    otherwise addresses that are never dereferenced."""
    if torch.cuda.is_available():
        pool = torch.zeros(17 * SLOT, dtype=torch.uint8, device="cuda")
        base = (pool.data_ptr() + SLOT - 1) // SLOT * SLOT
        torch.cuda.synchronize()
    else:
        pool, base = None, 0x7F0000000000
    return pool, [base + i * SLOT for i in range(16)]


WEIGHTS = (C.c_int32 * 65)()         # rvz_alphabeta's heuristic: host memory, read on the host

# name -> (arguments after (bs, n), the code for n = 0 with every pointer null)
#   "req": a pointer required when n > 0     "opt": a pointer that may be null
#   "w": rvz_alphabeta's weights (required whatever n is)     anything else: passed as it is
SOLVE = ["req", "req", "req", 10, C.c_int64(1000)]
WINDOW = [-64, 64, 0]
TABLE = {
    "rvz_board_legal": (["req", "req", "req", "req", None], OK),
    "rvz_board_apply": (["req", "req", "req", "req", "opt", None], OK),
    "rvz_board_canonical": (["req", "req", "req", "req", None], OK),
    "rvz_policy_softmax": (["req", "req", None], OK),
    "rvz_dirichlet_noise": (["req", "req", "req", 7, C.c_double(0.3), "req", "opt", None], OK),
    "rvz_action_probs": (["req", "req", "req", "req", "req", "opt", None], OK),
    "rvz_board_symmetry": (["req", "req", "req", "req", "req", None], OK),
    "rvz_training_rows": (["req", "req", "req", "req", "req", 1, "req", "req", "opt", None], OK),
    "rvz_training_rows/fan8": (["req", "req", "req", "req", "opt", 8, "req", "req", "opt", None],
                               OK),
    "rvz_merge_positions": (["req", "req", "req", "req", "req", 0, "req", "req", "req", "req",
                             "req", "req", "req", None], OK),
    "rvz_solve": (SOLVE + ["req", "req", "opt", None], OK),
    "rvz_solve_window": (SOLVE + WINDOW + ["req", "req", "opt", None], OK),
    "rvz_solve_moves": (SOLVE + WINDOW + ["req", "req", "opt", None], OK),
    "rvz_alphabeta": (["req", "req", "req", 4, "w", C.c_int64(1000), "req", "req", "opt", None],
                      EINVAL),
}


def _call(lib, name, bs, n, spec, ptrs, null=(), all_null=False):
    """null: indices (into spec) of the pointers passed as null; all_null: every pointer, the
    weights included."""
    args = []
    for i, a in enumerate(spec):
        if a in ("req", "opt"):
            args.append(None if all_null or i in null else ptrs[i])
        elif a == "w":
            args.append(None if all_null or i in null else C.addressof(WEIGHTS))
        else:
            args.append(a)
    return getattr(lib, name.split("/")[0])(bs, n, *args)


@pytest.mark.parametrize("name", sorted(TABLE))
def test_stateless_entry_points_check_their_arguments(lib, pointers, name):
    spec, at_zero = TABLE[name]
    _, ptrs = pointers
    optional = [i for i, a in enumerate(spec) if a == "opt"]
    for bs in (8, 6):
        # n = 0 with null pointers: the recorded answer, no launch
        assert _call(lib, name, bs, 0, spec, ptrs, all_null=True) == at_zero, (bs, "n = 0")
        # n = 0 with the optional pointers null and the others set: nothing to do
        assert _call(lib, name, bs, 0, spec, ptrs, null=optional) == OK, (bs, "n = 0, set")
        # n = -1
        assert _call(lib, name, bs, -1, spec, ptrs, null=optional) == EINVAL, (bs, "n = -1")
        # n = 1, each required pointer null in turn (the optional ones null throughout)
        for i, a in enumerate(spec):
            if a in ("req", "w"):
                assert _call(lib, name, bs, 1, spec, ptrs, null=optional + [i]) == EINVAL, (bs, i)
    # board size 7: refused whatever else is given (n = 0, so that a missing check would return
    # RVZ_OK here and launch nothing; n = 1 with the pointers set is refused by this check alone)
    assert _call(lib, name, 7, 0, spec, ptrs, null=optional) == EINVAL
    if not torch.cuda.is_available():
        assert _call(lib, name, 7, 1, spec, ptrs, null=optional) == EINVAL


# (board, filters) -> rvz_resnet_h2_grid(board, filters, 7), rvz_resnet_params_size(board, filters, 3)
RESNET = {
    (8, 64): (12, 248848), (8, 128): (15, 914768), (8, 256): (15, 3573712), (8, 96): (EINVAL, EINVAL),
    (6, 64): (11, 235996), (6, 128): (15, 901916), (6, 256): (EINVAL, 3560860), (6, 96): (EINVAL, EINVAL),
}


def test_resnet_size_and_grid_functions(lib):
    """The evaluator's size and grid functions for every (board, filters) of {6, 8} x {64, 128,
    256, 96}: the grid of 7 boards exists exactly where the trunk has a tile (not for 6x6 at 256,
    not for 96); the parameter count follows the width rule alone (it does not depend on a tile)."""
    for (board, f), (grid, params) in RESNET.items():
        assert lib.rvz_resnet_h2_grid(board, f, 7) == grid, (board, f)
        assert lib.rvz_resnet_params_size(board, f, 3) == params, (board, f)
        assert lib.rvz_resnet_h2_grid(board, f, -1) == EINVAL
        assert lib.rvz_resnet_h2_grid(board, f, 0) == (EINVAL if grid == EINVAL else 0)
        assert lib.rvz_resnet_params_size(board, f, -1) == EINVAL
    for f, size in ((64, 463776), (128, 1812256), (256, 7163424), (96, EINVAL)):
        assert lib.rvz_resnet_h2_size(f, 3) == size
        assert lib.rvz_resnet_h2_size(f, -1) == EINVAL
        assert lib.rvz_resnet_h2_grid(7, f, 7) == EINVAL
        assert lib.rvz_resnet_params_size(7, f, 3) == EINVAL
    assert lib.rvz_resnet_work_size(7) == 7 * 192 + 4 and lib.rvz_resnet_work_size(0) == 4
    assert lib.rvz_resnet_work_size(-1) == EINVAL
    # the launching entry points: a null pointer, a negative count, a pair without a tile and
    # n = 0 are all answered before HIP
    p = 0x10000
    for board, f, want in ((8, 64, OK), (6, 128, OK), (6, 256, EINVAL), (8, 96, EINVAL),
                           (7, 64, EINVAL)):
        assert lib.rvz_resnet_trunk_h2(board, p, 0, p, p, f, 1, p, None) == want, (board, f)
    assert lib.rvz_resnet_trunk_h2(8, p, -1, p, p, 64, 1, p, None) == EINVAL
    assert lib.rvz_resnet_trunk_h2(8, None, 0, p, p, 64, 1, p, None) == EINVAL
    assert lib.rvz_resnet_heads_fc(8, p, 0, p, 64, 1, p, p, None) == OK
    assert lib.rvz_resnet_heads_fc(7, p, 0, p, 64, 1, p, p, None) == EINVAL
    assert lib.rvz_resnet_heads_fc(6, p, 0, p, 256, 1, p, p, None) == OK      # the width rule
    assert lib.rvz_resnet_heads_fc(8, p, -1, p, 64, 1, p, p, None) == EINVAL
    assert lib.rvz_resnet_heads_fc(8, None, 0, p, 64, 1, p, p, None) == EINVAL
