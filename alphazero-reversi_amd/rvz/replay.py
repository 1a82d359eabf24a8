"""A replay buffer on the device: training batches sampled across iterations.

AlphaZero trains on minibatches drawn from a sliding window over the last K iterations of
self-play, not on one iteration's games alone. ``ReplayBuffer`` is that window: a ring of compact
records (mover bitboard, opponent bitboard, policy row, value: 280 B a row on 8x8 against the
1028 B of the expanded planes and policy) that ``records_to_training(..., compact=True)`` fills
and one HIP kernel samples (``rvz.replay_batch`` / rvz_replay_batch, include/rvz.h): a uniform
record and a fresh board symmetry per drawn row, the planes and the permuted policy written
straight from the bitboards, no host randomness.

``ReplayBuffer(weighted=True)`` adds a sampling weight per row (a merged position's record count,
a priority) and a recency decay, and draws rows in proportion to their weights: a table of integer
prefix sums built on the device after each append (``rvz.replay_cdf`` / rvz_replay_cdf) and one
kernel that draws through it (``rvz.replay_batch_weighted`` / rvz_replay_batch_weighted).

``ReplayBuffer(prioritized=True)`` is the prioritized replay of Schaul et al. (2016) on top of
that: new rows enter at the running maximum priority, ``update_priorities`` writes a trained
batch's losses back as the rows' weights (``rvz.replay_priority`` / rvz_replay_priority) and
``is_weights`` corrects the sampling bias in the loss (``rvz.replay_is_weight`` /
rvz_replay_is_weight).

``ReplayBuffer(stamps=True)`` adds a stamp per row, the iteration whose net produced the row's
policy target, and ``reanalyse``: the stalest rows are searched again with the current net and
their policy targets overwritten in place (MuZero's Reanalyse in an AlphaZero loop;
``rvz.replay_stale`` / ``rvz.replay_roots`` / ``rvz.replay_refresh``, csrc/rvz_reanalyse.hip).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from ._lib import RvzError, is_int, is_number
from .records import (check_priority_args, replay_batch, replay_batch_weighted, replay_cdf,
                      replay_is_weight, replay_ownership, replay_priority, replay_refresh,
                      replay_roots, replay_stale)


def check_recency_decay(recency_decay, name: str = "ReplayBuffer: recency_decay") -> None:
    """ReplayBuffer's rule for recency_decay (SelfPlayTrainer checks its replay_recency_decay by
    it too, under that name)."""
    if not is_number(recency_decay, 0.0, 1.0, lo_open=True):
        raise ValueError(f"{name} must be in (0, 1], not {recency_decay!r}")


class ReplayBuffer:
    ownership = False       # an instance attribute only with ownership=True

    def __init__(self, capacity: int, board_size: int = 8, device=None,
                 window_iterations: int = 0, batcher=None, weighted: bool = False,
                 recency_decay: float = 1.0, weighted_batcher=None, cdf_builder=None,
                 prioritized: bool = False, priority_alpha: float = 0.6,
                 priority_floor: float = 2.0 ** -8, priority_cap: float = 2.0 ** 8,
                 subtract_entropy: bool = True, priority_updater=None, is_weighter=None,
                 stamps: bool = False, ownership: bool = False, ownership_batcher=None):
        """capacity: the ring's rows. window_iterations = K > 0: an append of iteration t also
        drops every row of an iteration before t - K + 1 (0: rows leave only when overwritten).
        batcher(mover, opponent, policy, value, start, live, nb, seed, step, random_sym, idx, sym,
        board_size) -> (states, policy, value [nb, 1], slot, sym): default rvz.replay_batch (the
        rvz_replay_batch HIP kernel; the ring must then be on the GPU). Tests on a host without
        a GPU pass a NumPy restatement.
        The ledger of (iteration, rows) is kept on the host and row counts are tensor shapes, so
        neither append nor sample synchronises with the device.
        weighted=True: the ring also holds `weight` float32 [capacity], a sampling weight per row
        (append's `weight`, 1.0 by default), and sample draws a row with probability weight /
        the sum of the weights held. A weight counts in fixed point, rint(w * 2^16); one that is
        not finite or outside [0, 65536] counts as 0, so the row is never drawn
        (invalid_weights() counts them). recency_decay = d in (0, 1]: an append of an iteration t
        newer than the newest held iteration t0 first multiplies every held weight in place by
        float32(d ** (t - t0)), one float32 multiply per row, so a row's weight falls by d with
        every iteration it ages. The table of prefix sums the draw reads lives in a buffer
        allocated here once; append marks it stale and the next sample rebuilds it.
        cdf_builder(weight, start, live, tile_log2, out) -> the table built into `out`: default
        rvz.replay_cdf. weighted_batcher(mover, opponent, policy, value, cdf, start, live, nb,
        seed, step, random_sym, idx, sym, word, board_size) -> batcher's five outputs and prob
        [nb]: default rvz.replay_batch_weighted. total_weight() and invalid_weights() read the
        table's first two words: the only host synchronisations.
        prioritized=True (implies weighted): the weights are priorities driven by the training
        loss. An append without `weight` gives its rows the running maximum priority (one float32
        on the device, 1.0 at first, broadcast into the slice without a host synchronisation), so
        a new row is drawn at least as readily as any held row until it has been trained on once;
        an explicit `weight` still wins. update_priorities(slot, rows) then writes
        min(priority_cap, max(priority_floor, e ** priority_alpha)) into the slots of a trained
        batch, e = policy_coef * k + value_coef * Lv of the batch's loss rows, k the policy's KL
        divergence from its target with subtract_entropy (the default: the cross-entropy Lp alone
        can never reach 0 on a high-entropy target and would favour opening rows for ever), Lp
        without. priority_alpha = 0.6 is the value of Schaul et al. (0: uniform sampling);
        priority_floor = 2^-8 and priority_cap = 2^8 are choices, not measurements: a span of
        2^16 between the rarest and the commonest held row, inside the fixed point's [2^-16, 2^16].
        recency_decay multiplies the held weights as before and leaves the running maximum alone.
        priority_updater(weight, slot, rows, policy_coef, value_coef, subtract_entropy, alpha,
        floor, cap, max_priority) -> (priority, state), writing weight and max_priority in place:
        default rvz.replay_priority. is_weighter(prob, slot, beta) -> weight: default
        rvz.replay_is_weight.
        stamps=True: the ring also holds `stamp` int32 [capacity], the iteration whose net
        produced each row's policy target: append's `stamp` (default: its iteration), and what
        reanalyse() selects by and rewrites. Without it the buffer allocates nothing more and
        behaves exactly as before.
        ownership=True: the ring also holds `final_mover` and `final_opponent` int64 [capacity],
        the final position of each row's game from the row's mover's side (16 B a row; append's
        arguments of those names, rvz.records_final's outputs), and sample returns two more
        outputs at its end: ownership float32 [nb, S*S] (+1 / -1 / 0: who holds each square at the
        end of the game, under the drawn row's own symmetry) and margin float32 [nb] (the final
        disc margin), under the uniform, weighted and prioritized draws alike.
        ownership_batcher(final_mover, final_opponent, slot, sym, board_size) -> (ownership,
        margin): default rvz.replay_ownership (the rvz_replay_ownership HIP kernel), called on
        the draw's own slot and sym. reanalyse leaves the two columns alone. Without it the buffer
        allocates nothing more and behaves exactly as before."""
        for name, x in (("capacity", capacity), ("window_iterations", window_iterations)):
            if not is_int(x):
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
        self.prioritized = bool(prioritized)
        self.weighted = bool(weighted) or self.prioritized
        if not self.prioritized and (priority_updater is not None or is_weighter is not None or
                                     (priority_alpha, priority_floor, priority_cap) !=
                                     (0.6, 2.0 ** -8, 2.0 ** 8) or subtract_entropy is not True):
            raise ValueError("ReplayBuffer: priority_alpha, priority_floor, priority_cap, "
                             "subtract_entropy, priority_updater and is_weighter need "
                             "prioritized=True")
        if not self.weighted and (recency_decay != 1.0 or weighted_batcher is not None or
                                  cdf_builder is not None):
            raise ValueError("ReplayBuffer: recency_decay, weighted_batcher and cdf_builder need "
                             "weighted=True")
        check_recency_decay(recency_decay)
        if ownership_batcher is not None and not ownership:
            raise ValueError("ReplayBuffer: ownership_batcher needs ownership=True")
        self.mover, self.opponent = self._zeros(torch.int64), self._zeros(torch.int64)
        self.policy = self._zeros(torch.float32, self.board_size ** 2 + 1)
        self.value = self._zeros(torch.float32)
        self.start = 0                  # the slot of the oldest row
        self._live = 0
        self._ledger: List[List[int]] = []      # [iteration, rows], oldest first
        self.stamps = bool(stamps)
        if self.stamps:
            self.stamp = self._zeros(torch.int32)
        if ownership:
            self.ownership = True
            self.ownership_batcher = (replay_ownership if ownership_batcher is None
                                      else ownership_batcher)
            self.final_mover, self.final_opponent = (self._zeros(torch.int64),
                                                     self._zeros(torch.int64))
        if self.weighted:
            self.recency_decay = float(recency_decay)
            self.weighted_batcher = (replay_batch_weighted if weighted_batcher is None
                                     else weighted_batcher)
            self.cdf_builder = replay_cdf if cdf_builder is None else cdf_builder
            self.weight = self._zeros(torch.float32)
            # the table at this capacity: 4 words of header, one per row, the scan's upper levels
            words = _lib.load().rvz_replay_cdf_size(self.capacity, 0) // 8
            self._cdf = torch.zeros(words, dtype=torch.int64, device=self.device)
            self._dirty = True
        if self.prioritized:
            try:                        # the rules of rvz.replay_priority, on an empty batch
                check_priority_args(self.weight, torch.zeros(0, dtype=torch.int32),
                                    torch.zeros(0, 3, dtype=torch.float64), 1.0, 1.0,
                                    subtract_entropy, priority_alpha, priority_floor,
                                    priority_cap, who="ReplayBuffer")
            except RvzError as err:
                raise ValueError(str(err)) from None
            self.priority_alpha = float(priority_alpha)
            self.priority_floor, self.priority_cap = float(priority_floor), float(priority_cap)
            self.subtract_entropy = bool(subtract_entropy)
            self.priority_updater = replay_priority if priority_updater is None \
                else priority_updater
            self.is_weighter = replay_is_weight if is_weighter is None else is_weighter
            self._max_priority = torch.ones(1, dtype=torch.float32, device=self.device)

    def _zeros(self, dtype, *row_shape) -> torch.Tensor:
        return torch.zeros(self.capacity, *row_shape, dtype=dtype, device=self.device)

    def _columns(self) -> Dict[str, torch.Tensor]:
        """The ring's per-row columns, name -> tensor [capacity, ...], in append's write order.
        Each is the attribute of its name, there only with the option it belongs to."""
        return {k: vars(self)[k] for k in ("mover", "opponent", "policy", "value", "final_mover",
                                           "final_opponent", "weight", "stamp") if k in vars(self)}

    def _write(self, ring: torch.Tensor, head: int, n: int, rows) -> None:
        """rows (a tensor of n rows, or one scalar for all n) into the n slots from `head` on,
        wrapping at the ring's end: at most two slice writes."""
        first = min(n, self.capacity - head)
        tensor = isinstance(rows, torch.Tensor)
        ring[head:head + first] = rows[:first] if tensor else rows
        if first < n:
            ring[:n - first] = rows[first:] if tensor else rows

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
               value: torch.Tensor, iteration: int,
               weight: Optional[torch.Tensor] = None, stamp: Optional[int] = None,
               final_mover: Optional[torch.Tensor] = None,
               final_opponent: Optional[torch.Tensor] = None) -> None:
        """n <= capacity rows of `iteration` at the head of the ring (at most two slice copies per
        tensor), over the oldest rows once the ring is full. mover / opponent int64 [n], policy
        float32 [n, S*S+1], value float32 [n] or [n, 1]. Iterations are appended in
        non-decreasing order. weight (weighted=True only): float32 [n], the rows' sampling
        weights; None: 1.0 each (prioritized=True: the running maximum priority each). stamp
        (stamps=True only): the iteration whose net produced the rows' policy targets, an int in
        [0, 2^31); None: `iteration`. final_mover / final_opponent (ownership=True only, and
        required then): int64 [n], the rows' final positions."""
        if not is_int(iteration):
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
        if weight is not None:
            if not self.weighted:
                raise ValueError("ReplayBuffer.append: weight needs ReplayBuffer(weighted=True)")
            if weight.shape != (n,) or weight.dtype != torch.float32:
                raise ValueError("ReplayBuffer.append: weight is float32 [n]")
        if (final_mover is not None or final_opponent is not None) and not self.ownership:
            raise ValueError("ReplayBuffer.append: final_mover and final_opponent need "
                             "ReplayBuffer(ownership=True)")
        if self.ownership:
            for t in (final_mover, final_opponent):
                if not isinstance(t, torch.Tensor) or t.shape != (n,) or t.dtype != torch.int64:
                    raise ValueError("ReplayBuffer.append: a ReplayBuffer(ownership=True) takes "
                                     "final_mover and final_opponent, int64 [n]")
        if stamp is not None and not self.stamps:
            raise ValueError("ReplayBuffer.append: stamp needs ReplayBuffer(stamps=True)")
        if self.stamps:
            stamp = iteration if stamp is None else stamp
            if not is_int(stamp) or not 0 <= stamp < 2 ** 31:
                raise ValueError(f"ReplayBuffer.append: stamp is an int in [0, 2^31), not "
                                 f"{stamp!r}")
        if n > self.capacity:
            raise ValueError(f"ReplayBuffer.append: {n} rows do not fit a ring of {self.capacity}")
        if self._ledger and iteration < self._ledger[-1][0]:
            raise ValueError(f"ReplayBuffer.append: iteration {iteration} after iteration "
                             f"{self._ledger[-1][0]}")
        if n:
            head = (self.start + self._live) % self.capacity
            rows = {"mover": mover, "opponent": opponent, "policy": policy,
                    "value": value.reshape(n), "final_mover": final_mover,
                    "final_opponent": final_opponent}
            if self.weighted:
                if self._ledger and iteration > self._ledger[-1][0] and self.recency_decay != 1.0:
                    # the held rows age by the iterations that passed (slots that hold no row too:
                    # they are never read)
                    factor = self.recency_decay ** (int(iteration) - self._ledger[-1][0])
                    self.weight.mul_(torch.tensor(factor, dtype=torch.float32).item())
                if weight is None and self.prioritized:
                    weight = self._max_priority.expand(n)       # read on the device
                elif weight is None:
                    weight = torch.ones(n, dtype=torch.float32, device=self.device)
                rows["weight"] = weight
                self._dirty = True
            if self.stamps:
                rows["stamp"] = int(stamp)
            for name, ring in self._columns().items():
                self._write(ring, head, n, rows[name])
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
                if self.weighted:
                    self._dirty = True

    def sample(self, nb: int, seed: int, step: int, symmetries: bool = True,
               idx: Optional[torch.Tensor] = None, sym: Optional[torch.Tensor] = None,
               word: Optional[torch.Tensor] = None, with_prob: bool = False):
        """A batch of nb rows: (states [nb, 3, S, S], policy [nb, S*S+1], value [nb, 1], slot
        [nb], sym [nb]), a pure function of (the ring, seed, step). Every row is drawn uniformly
        from the rows held, under a uniformly drawn board symmetry (symmetries=False: the
        identity). idx / sym [nb]: the logical rows (0 the oldest) and the symmetries to take
        instead of the draws.
        weighted=True: every row is drawn with probability weight / total weight instead (the
        symmetries are the same draws). word [nb] int64 (uint64 bit patterns): the uniform 64-bit
        words to draw with in place of the generator's. with_prob=True: a sixth output, prob
        float32 [nb], each taken row's probability. With every weight 0 or invalid all drawn rows
        are zero rows with slot -1 and sym -1.
        ownership=True: two more outputs after those, ownership float32 [nb, S*S] and margin
        float32 [nb], the drawn rows' ownership targets under their own symmetries (zero for a
        zero row)."""
        out = self._draw(nb, seed, step, symmetries, idx, sym, word, with_prob)
        if self.ownership:
            out = (*out, *self.ownership_batcher(self.final_mover, self.final_opponent, out[3],
                                                 out[4], self.board_size))
        return out

    def _draw(self, nb, seed, step, symmetries, idx, sym, word, with_prob):
        if not self._live:
            raise ValueError("ReplayBuffer.sample: the buffer is empty")
        if self.weighted:
            out = self.weighted_batcher(self.mover, self.opponent, self.policy, self.value,
                                        self._table(), self.start, self._live, nb, seed, step,
                                        bool(symmetries), idx, sym, word, self.board_size)
            return out if with_prob else out[:5]
        if word is not None or with_prob:
            raise ValueError("ReplayBuffer.sample: word and with_prob need "
                             "ReplayBuffer(weighted=True)")
        return self.batcher(self.mover, self.opponent, self.policy, self.value, self.start,
                            self._live, nb, seed, step, bool(symmetries), idx, sym,
                            self.board_size)

    def _table(self) -> torch.Tensor:
        """The table of the rows held now, rebuilt if an append changed them."""
        if self._dirty:
            self._cdf = self.cdf_builder(self.weight, self.start, self._live, 0, self._cdf)
            self._dirty = False
        return self._cdf

    def total_weight(self) -> float:
        """The sum of the valid weights held, as sampled: fixed point / 2^16. Synchronises."""
        if not self.weighted:
            raise ValueError("ReplayBuffer.total_weight needs ReplayBuffer(weighted=True)")
        return int(self._table()[0].item()) / 65536.0 if self._live else 0.0

    def invalid_weights(self) -> int:
        """The rows held whose weight is not finite or outside [0, 65536]: they are never drawn.
        Synchronises."""
        if not self.weighted:
            raise ValueError("ReplayBuffer.invalid_weights needs ReplayBuffer(weighted=True)")
        return int(self._table()[1].item()) if self._live else 0

    def _need_priorities(self, who: str) -> None:
        if not self.prioritized:
            raise ValueError(f"ReplayBuffer.{who} needs ReplayBuffer(prioritized=True)")

    def update_priorities(self, slot: torch.Tensor, rows: torch.Tensor, policy_coef: float = 1.0,
                          value_coef: float = 1.0):
        """A trained batch's losses as its rows' new sampling weights: slot [nb] the batch's
        slots (sample's fourth output), rows float64 [nb, 3] its loss rows {Lp, Lv, H}
        (full_policy_loss(rows=True)'s stats["rows"]), policy_coef / value_coef the loss's own
        weights. Where a slot was drawn more than once the last row's priority is written; a
        row with slot -1 or a non-finite loss writes nothing. Raises the running maximum and
        marks the table stale (the next sample rebuilds it). No append may have come between the
        draw and this call. Returns (priority float32 [nb], state int32 [nb]: 1 written, 0
        superseded, -1 invalid). Nothing synchronises."""
        self._need_priorities("update_priorities")
        out = self.priority_updater(self.weight, slot, rows, policy_coef, value_coef,
                                    self.subtract_entropy, self.priority_alpha,
                                    self.priority_floor, self.priority_cap, self._max_priority)
        self._dirty = True
        return out

    def is_weights(self, prob: torch.Tensor, slot: torch.Tensor, beta: float) -> torch.Tensor:
        """The importance-sampling weights of a drawn batch, float32 [nb]: (pmin / prob) ** beta,
        1 at the rarest drawn row, 0 at a zero row (sample(with_prob=True)'s prob and slot)."""
        self._need_priorities("is_weights")
        return self.is_weighter(prob, slot, beta)

    def max_priority(self) -> float:
        """The running maximum priority: what the next appended row enters at. Synchronises."""
        self._need_priorities("max_priority")
        return float(self._max_priority.item())

    def rows_leaving(self, iteration: int) -> int:
        """The oldest rows held that an append of `iteration` would drop through
        window_iterations (0 without a window): the rows of every iteration before
        iteration - window_iterations + 1. Rows that leave because the head runs over them in a
        full ring are not counted: that depends on the size of the append."""
        if not self.window_iterations:
            return 0
        return sum(rows for it, rows in self._ledger
                   if it < iteration - self.window_iterations + 1)

    def reanalyse(self, engine, evaluator, rows: int, lo: int, below: int, new_stamp: int,
                  with_old: bool = False, first: int = 0):
        """Replay reanalysis: up to `rows` of the stalest rows held (stamp below `below`, the
        stamps at or below `lo` counting as equally stale; rvz.replay_stale) are searched again by
        `engine` with `evaluator`, the current net, and their policy targets and stamps are
        overwritten in place with the new search's visit distributions and new_stamp. In chunks
        of engine.n_games rows, the last one padded with -1: rvz.replay_roots, engine.set_state,
        engine.memo_reset() where the memo is on, engine.search(evaluator), engine.act(1.0,
        apply=False) with a given draw (the act's probability rows do not depend on it, and the
        engine's own draw streams stay where they are), rvz.replay_refresh. The pull-style search
        is the one that runs, not the fused rvz_play. value, mover and opponent are not touched:
        the outcome of the game does not depend on the net.
        The ring's sampling weights are not touched either. A merged row's fresh policy replaces
        the mean policy of its records, and the row keeps its record count as its weight. In a
        prioritized ring the row keeps its priority, and the next training step that draws it sets
        a new one from its loss against the fresh target.
        Returns a dict of device tensors, nothing synchronised beyond set_state's own wait:
        first: the selection leaves out the `first` oldest rows held (0 <= first <= len(self)):
        rows_leaving(t + 1) of them when the rows are next trained on after an append of
        iteration t + 1, which drops those rows unread.
        "slot" int32 [rows] (the selected slots, oldest first, then -1), "selected" int32 [2]
        (replay_stale's count: the rows selected, the held rows with a negative stamp), "counts"
        int64 [2] (the slots written, the rows skipped, padding included), "bad" int64 [1]
        (replay_roots' count), and with with_old=True "old_policy" float32 [rows, S*S+1]: the
        selected rows' targets before the refresh (a row of slot -1 holds slot 0's).
        ValueError: a buffer without stamps=True, an engine with root noise, an opening pool or a
        temperature schedule set (the re-search must be the plain search at temperature 1), or
        one whose board size differs from the ring's."""
        who = "ReplayBuffer.reanalyse"
        if not self.stamps:
            raise ValueError(f"{who} needs ReplayBuffer(stamps=True)")
        noise = getattr(engine, "noise", None)
        if noise is not None and noise[1] != 0.0:
            raise ValueError(f"{who}: the engine has root noise set")
        if getattr(engine, "pool", None) is not None:
            raise ValueError(f"{who}: the engine has an opening pool set")
        if getattr(engine, "schedule", None) is not None:
            raise ValueError(f"{who}: the engine has a temperature schedule set")
        if engine.board_size != self.board_size:
            raise ValueError(f"{who}: the engine plays {engine.board_size}x{engine.board_size}, "
                             f"the ring holds {self.board_size}x{self.board_size}")
        for name, x in (("rows", rows), ("lo", lo), ("below", below), ("new_stamp", new_stamp)):
            if not is_int(x):
                raise ValueError(f"{who}: {name} is an int, not {x!r}")
        if not is_int(first) or not 0 <= first <= self._live:
            raise ValueError(f"{who}: first = {first!r} must be an int in [0, {self._live}]")
        rows, G, first = int(rows), engine.n_games, int(first)
        out = {"slot": torch.full((max(rows, 0),), -1, dtype=torch.int32, device=self.device),
               "selected": torch.zeros(2, dtype=torch.int32, device=self.device),
               "counts": torch.zeros(2, dtype=torch.int64, device=self.device),
               "bad": torch.zeros(1, dtype=torch.int64, device=self.device)}
        if with_old:
            out["old_policy"] = torch.zeros(max(rows, 0), self.policy.shape[1],
                                            dtype=torch.float32, device=self.device)
        if self._live == first or rows <= 0:
            if rows < 0:
                raise ValueError(f"{who}: rows must be >= 0")
            return out
        try:
            slot, out["selected"] = replay_stale(self.stamp, (self.start + first) % self.capacity,
                                                 self._live - first, rows, lo, below)
        except RvzError as err:
            raise ValueError(str(err)) from None
        out["slot"] = slot
        if with_old:
            out["old_policy"] = self.policy[slot.clamp(min=0).long()]
        pad = (-rows) % G
        if pad:
            slot = torch.cat([slot, torch.full((pad,), -1, dtype=torch.int32,
                                               device=self.device)])
        u = torch.full((G,), 0.5, dtype=torch.float64, device=self.device)
        for at in range(0, rows, G):
            chunk = slot[at:at + G]
            black, white, status, bad = replay_roots(self.mover, self.opponent, chunk,
                                                     self.board_size)
            engine.set_state(black, white, status)
            if engine.memo_on:
                engine.memo_reset()
            engine.search(evaluator)
            idx, p = engine.act(1.0, u=u, apply=False)
            counts = replay_refresh(self.policy, self.stamp, chunk, p, idx, new_stamp)
            out["counts"] += counts
            out["bad"] += bad
        return out
