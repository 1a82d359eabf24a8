"""A replay buffer on the device: training batches sampled across iterations.

AlphaZero trains on minibatches drawn from a sliding window over the last K iterations of
self-play, not on one iteration's games alone. ``ReplayBuffer`` is that window: a ring of compact
records (mover bitboard, opponent bitboard, policy row, value: 280 B a row on 8x8 against the
1028 B of the expanded planes and policy) that ``records_to_training(..., compact=True)`` fills
and one HIP kernel samples (``rvz.replay_batch`` / rvz_replay_batch, include/rvz.h): a uniform
record and a fresh board symmetry per drawn row, the planes and the permuted policy written
straight from the bitboards, no host randomness.
"""
from __future__ import annotations

import numbers
from typing import List, Optional, Tuple

import torch

from .engine import replay_batch


class ReplayBuffer:
    def __init__(self, capacity: int, board_size: int = 8, device=None,
                 window_iterations: int = 0, batcher=None):
        """capacity: the ring's rows. window_iterations = K > 0: an append of iteration t also
        drops every row of an iteration before t - K + 1 (0: rows leave only when overwritten).
        batcher(mover, opponent, policy, value, start, live, nb, seed, step, random_sym, idx, sym,
        board_size) -> (states, policy, value [nb, 1], slot, sym): default rvz.replay_batch (the
        rvz_replay_batch HIP kernel; the ring must then be on the GPU). Tests on a host without
        a GPU pass a NumPy restatement.
        The ledger of (iteration, rows) is kept on the host and row counts are tensor shapes, so
        neither append nor sample synchronises with the device."""
        for name, x in (("capacity", capacity), ("window_iterations", window_iterations)):
            if isinstance(x, bool) or not isinstance(x, numbers.Integral):
                raise ValueError(f"ReplayBuffer: {name} is an int, not {x!r}")
        if board_size not in (8, 6):
            raise ValueError("board_size must be 8 or 6")
        if not 1 <= capacity < 2 ** 31:
            raise ValueError("ReplayBuffer: capacity must be in [1, 2^31)")
        if window_iterations < 0:
            raise ValueError("ReplayBuffer: window_iterations must be >= 0")
        self.capacity, self.board_size = int(capacity), int(board_size)
        self.window_iterations = int(window_iterations)
        self.device = torch.device("cuda" if device is None else device)
        self.batcher = replay_batch if batcher is None else batcher
        npol = self.board_size ** 2 + 1
        self.mover = torch.zeros(self.capacity, dtype=torch.int64, device=self.device)
        self.opponent = torch.zeros(self.capacity, dtype=torch.int64, device=self.device)
        self.policy = torch.zeros(self.capacity, npol, dtype=torch.float32, device=self.device)
        self.value = torch.zeros(self.capacity, dtype=torch.float32, device=self.device)
        self.start = 0                  # the slot of the oldest row
        self._live = 0
        self._ledger: List[List[int]] = []      # [iteration, rows], oldest first

    def __len__(self) -> int:
        return self._live

    def rows_by_iteration(self) -> List[Tuple[int, int]]:
        """(iteration, rows held) of every iteration with a row in the ring, oldest first."""
        return [(it, n) for it, n in self._ledger]

    def _drop_oldest(self, rows: int) -> None:
        self.start = (self.start + rows) % self.capacity
        self._live -= rows
        while rows:
            take = min(rows, self._ledger[0][1])
            self._ledger[0][1] -= take
            rows -= take
            if not self._ledger[0][1]:
                self._ledger.pop(0)

    def append(self, mover: torch.Tensor, opponent: torch.Tensor, policy: torch.Tensor,
               value: torch.Tensor, iteration: int) -> None:
        """n <= capacity rows of `iteration` at the head of the ring (at most two slice copies per
        tensor), over the oldest rows once the ring is full. mover / opponent int64 [n], policy
        float32 [n, S*S+1], value float32 [n] or [n, 1]. Iterations are appended in
        non-decreasing order."""
        if isinstance(iteration, bool) or not isinstance(iteration, numbers.Integral):
            raise ValueError(f"ReplayBuffer.append: iteration is an int, not {iteration!r}")
        n = mover.numel()
        npol = self.board_size ** 2 + 1
        if mover.dim() != 1 or opponent.shape != (n,) or policy.shape != (n, npol) or \
                value.shape not in ((n,), (n, 1)):
            raise ValueError(f"ReplayBuffer.append: mover and opponent [n], policy [n, {npol}], "
                             "value [n] or [n, 1]")
        if mover.dtype != torch.int64 or opponent.dtype != torch.int64 or \
                policy.dtype != torch.float32 or value.dtype != torch.float32:
            raise ValueError("ReplayBuffer.append: mover and opponent are int64, policy and value "
                             "float32")
        if n > self.capacity:
            raise ValueError(f"ReplayBuffer.append: {n} rows do not fit a ring of {self.capacity}")
        if self._ledger and iteration < self._ledger[-1][0]:
            raise ValueError(f"ReplayBuffer.append: iteration {iteration} after iteration "
                             f"{self._ledger[-1][0]}")
        if n:
            head = (self.start + self._live) % self.capacity
            first = min(n, self.capacity - head)
            for ring, rows in ((self.mover, mover), (self.opponent, opponent),
                               (self.policy, policy), (self.value, value.reshape(n))):
                ring[head:head + first].copy_(rows[:first])
                if first < n:
                    ring[:n - first].copy_(rows[first:])
            if self._ledger and self._ledger[-1][0] == iteration:
                self._ledger[-1][1] += n
            else:
                self._ledger.append([int(iteration), n])
            self._live += n
            if self._live > self.capacity:              # the head ran over the oldest rows
                self._drop_oldest(self._live - self.capacity)
        if self.window_iterations:
            old = sum(rows for it, rows in self._ledger
                      if it < iteration - self.window_iterations + 1)
            if old:
                self._drop_oldest(old)

    def sample(self, nb: int, seed: int, step: int, symmetries: bool = True,
               idx: Optional[torch.Tensor] = None, sym: Optional[torch.Tensor] = None):
        """A batch of nb rows: (states [nb, 3, S, S], policy [nb, S*S+1], value [nb, 1], slot
        [nb], sym [nb]), a pure function of (the ring, seed, step). Every row is drawn uniformly
        from the rows held, under a uniformly drawn board symmetry (symmetries=False: the
        identity). idx / sym [nb]: the logical rows (0 the oldest) and the symmetries to take
        instead of the draws."""
        if not self._live:
            raise ValueError("ReplayBuffer.sample: the buffer is empty")
        return self.batcher(self.mover, self.opponent, self.policy, self.value, self.start,
                            self._live, nb, seed, step, bool(symmetries), idx, sym,
                            self.board_size)
