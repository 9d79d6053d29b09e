"""The learner's side of self-play: the replay buffer's tensors and the batches drawn from them; no engine needed.

For a learner on the same GPU the finished games need not leave HBM at all: `ReplayTensors` is the reference
learner's dense buffer layout (ReplayBuffer.py:11-23), `NativeSelfPlay.export(buffer)` (src/selfplay.py) writes the
finished store into it as replay rows with one kernel (k_sp_export through az_selfplay_export: what game.py:110-157
followed by ReplayBuffer.py:92-123 would leave there), and `ReplayTensors.store_games(drain())` is the same
thing by the host route, for any driver.

The way out of that buffer stays on the device too: `SampledReplayTensors.sample(batch_size)` draws a sample as the
reference's `ReplayBuffer.sample` sizes it and returns the epochs' batches (`ReplayBatches`), each batch gathered,
cast and symmetry-augmented by one kernel (k_replay_batch through az_replay_dev_batch, csrc/replay_kernels.hip) in
place of the reference's DataLoader and per-batch `augment`; `ReplayTensors.batches(indices, ...)` is the same
iteration over indices of the caller's, and `augmented` the identity to pass as `augment` to a training step.
"""

import ctypes as C

import numpy as np
import torch

from src.abi import ReplayBatchC, ReplayTensorsC, _stream, check, lib

REPLAY_GEOMETRY = {"Connect4": (7, 6, 7), "Othello": (65, 8, 8)}       # actions, rows, columns


class ReplayTensors:
    """The dense tensors the reference's learner keeps its positions in (ReplayBuffer.py:11-23), as a plain
    container: same attribute names, dtypes and shapes, the ring rule of `store` (ReplayBuffer.py:92-123: row
    number `_ptr` goes to index `_ptr % current_capacity`), `__len__` and `get`.  Persistence and the replay
    ratio are the learner's and are not here; the reference's `sample` is `SampledReplayTensors.sample`.  `state`
    and `prob`, which the reference leaves uninitialised, start as zeros; the rest starts as the reference's does.

    Rows arrive from `NativeSelfPlay.export(self)` (on the device, no host copy) or `store_games(drain())` (any
    driver, any device, the CPU included) and leave as augmented training batches through `batches`."""

    def __init__(self, game, capacity, device="cpu"):
        assert game in REPLAY_GEOMETRY and int(capacity) > 0
        A, R, Cc = REPLAY_GEOMETRY[game]
        cap = int(capacity)
        self.game = game
        self.device = torch.device(device)
        z = dict(device=self.device)
        self.state = torch.zeros((cap, 3, R, Cc), dtype=torch.int8, **z)
        self.prob = torch.zeros((cap, A), dtype=torch.float32, **z)
        self.winner = torch.zeros((cap, 1), dtype=torch.int8, **z)
        self.steps_to_end = torch.zeros((cap, 1), dtype=torch.int16, **z)
        self.aux_target = torch.zeros((cap, 1), dtype=torch.int16, **z)
        self.root_wdl = torch.zeros((cap, 3), dtype=torch.float32, **z)
        self.future_root_wdl = torch.zeros((cap, 3), dtype=torch.float32, **z)
        self.valid_mask = torch.ones((cap, A), dtype=torch.bool, **z)
        self.current_capacity = cap
        self._ptr = 0

    TENSORS = ("state", "prob", "winner", "steps_to_end", "aux_target", "root_wdl", "valid_mask", "future_root_wdl")

    def __len__(self):
        return min(self._ptr, len(self.state))

    def get(self, indices):
        return (self.state[indices].float(), self.prob[indices], self.winner[indices], self.steps_to_end[indices],
                self.aux_target[indices], self.root_wdl[indices], self.valid_mask[indices], self.future_root_wdl[indices])

    def batches(self, indices, batch_size, order=None, drop_last=False, route=None):
        """The rows `indices` (int64, any sequence or tensor) as augmented training batches of `batch_size` samples:
        a `ReplayBatches` in the order given, or in `order` (a permutation of the positions of `indices`).  The last
        batch is short unless `drop_last`.  `route`: "kernel" (k_replay_batch; the default on a GPU), "torch" (plain
        indexing, flips and concatenation; the only route on the CPU)."""
        return ReplayBatches(self, indices, batch_size, order=order, drop_last=drop_last, route=route)

    def store_games(self, games):
        """The host route: `games` as any driver's `drain()` returns them, a list of (winner, play_data, slot);
        every tuple of every play_data becomes one row, in order, as `buffer.store(*data)` per tuple would
        (server.py:300-302).  One indexed assignment per column and game.  Returns the rows stored."""
        cap = self.current_capacity
        n_rows = 0
        for _winner, play, *_ in games:
            n = len(play)
            cols = list(zip(*play))
            keep = slice(max(0, n - cap), n)              # a game longer than the ring: its last rows survive
            idx = torch.from_numpy(((self._ptr + np.arange(n, dtype=np.int64)) % cap)[keep]).to(self.device)

            def put(dst, col, dtype):
                a = np.ascontiguousarray(np.stack([np.asarray(x) for x in col[keep]]).astype(dtype, copy=False))
                dst[idx] = torch.from_numpy(a).to(self.device).reshape((len(a),) + tuple(dst.shape[1:]))
            put(self.state, cols[0], np.int8)
            put(self.prob, cols[1], np.float32)
            put(self.winner, cols[2], np.int8)
            put(self.steps_to_end, cols[3], np.int16)
            put(self.aux_target, cols[4], np.int16)
            put(self.root_wdl, cols[5], np.float32)
            put(self.valid_mask, cols[6], np.bool_)
            if len(cols) > 7:
                put(self.future_root_wdl, cols[7], np.float32)
            else:
                self.future_root_wdl[idx] = 0
            self._ptr += n
            n_rows += n
        return n_rows


def replay_tensors_c(buffer, game, device, who="export"):
    """az_replay_tensors of `buffer` (a ReplayTensors or anything with its attributes, the reference's
    ReplayBuffer included) after checking that the kernels may use it (k_sp_export writes it, k_replay_batch
    reads it): ValueError otherwise."""
    A, R, Cc = REPLAY_GEOMETRY[game]
    try:
        cap = int(buffer.current_capacity)
        tensors = {n: getattr(buffer, n) for n in ReplayTensors.TENSORS}
        int(buffer._ptr)
    except AttributeError as e:
        raise ValueError("%s: the buffer lacks %s" % (who, e))
    if cap <= 0:
        raise ValueError("%s: the buffer's capacity must be positive" % who)
    want = dict(state=(torch.int8, (3, R, Cc)), prob=(torch.float32, (A,)), winner=(torch.int8, (1,)),
                steps_to_end=(torch.int16, (1,)), aux_target=(torch.int16, (1,)), root_wdl=(torch.float32, (3,)),
                valid_mask=(torch.bool, (A,)), future_root_wdl=(torch.float32, (3,)))
    dev = torch.device(device)
    for n, t in tensors.items():
        dtype, tail = want[n]
        if not isinstance(t, torch.Tensor) or t.device.type != dev.type or (dev.index is not None and t.device.index != dev.index):
            raise ValueError("%s: buffer.%s is not a tensor on %s" % (who, n, dev))
        if t.dtype != dtype or tuple(t.shape[1:]) != tail:
            raise ValueError("%s: buffer.%s must be %s [capacity]%s, not %s %s" % (who, n, dtype, list(tail), t.dtype, list(t.shape)))
        if not t.is_contiguous() or t.data_ptr() % 16:
            raise ValueError("%s: buffer.%s must be contiguous and 16-byte aligned" % (who, n))
        if t.shape[0] < cap:
            raise ValueError("%s: buffer.%s has %d rows, fewer than current_capacity %d" % (who, n, t.shape[0], cap))
    return ReplayTensorsC(*(tensors[n].data_ptr() for n in ReplayTensors.TENSORS), cap)


def sample_size(total, batch_size, full_batches=False, replay_ratio=0.25):
    """Rows the reference's `ReplayBuffer.sample` draws from a buffer of `total` rows (ReplayBuffer.py:131-140):
    `replay_ratio` of them once the buffer holds more than 10000 / replay_ratio, at most 10000 before; with
    `full_batches` rounded down to whole batches, one batch at least."""
    total = int(total)
    assert total > 0
    n = int(total * replay_ratio) if total > 10000 / replay_ratio else min(total, 10000)
    if full_batches:
        batch_size = int(batch_size)
        if batch_size <= 0:
            raise ValueError("batch_size must be positive")
        n = max(batch_size, (n // batch_size) * batch_size)
    return n


def _seed63(seed, call):
    return (int(seed) * 0x9E3779B97F4A7C15 + int(call) * 0xBF58476D1CE4E5B9 + 1) & (2 ** 63 - 1)


def _augment_torch(game, state, prob, mask):
    """The game's board symmetries, stacked symmetry-major, in plain torch.  Connect4: identity, c -> 6 - c.
    Othello: identity, (r, c) -> (7 - r, 7 - c), (r, c) -> (c, r), (r, c) -> (7 - c, 7 - r); the pass entry stays.
    Planes 0 and 1 of `state` move, plane 2 (the turn sign) does not."""
    stones, turn = state[:, :2], state[:, 2:]
    if game == "Connect4":
        return (torch.cat([state, torch.cat([stones.flip(3), turn], 1)]), torch.cat([prob, prob.flip(1)]),
                torch.cat([mask, mask.flip(1)]))

    def images(x):                                   # x: [n, ..., 8, 8]
        turned = x.flip(-2, -1)
        return [turned, x.transpose(-2, -1), turned.transpose(-2, -1)]

    def actions(x):                                  # x: [n, 65]
        n = x.shape[0]
        return [x] + [torch.cat([b.reshape(n, 64), x[:, 64:]], 1) for b in images(x[:, :64].reshape(n, 8, 8))]
    return (torch.cat([state] + [torch.cat([b, turn], 1) for b in images(stones)]), torch.cat(actions(prob)),
            torch.cat(actions(mask)))


def augmented(batch):
    """The identity: the `augment` to hand a training step whose loader (`ReplayBatches`) augments already."""
    return batch


class ReplayBatches:
    """The batches of one sample of a replay buffer; re-iterable, one epoch per `__iter__`.

    `indices`: the sampled ring rows (exposed as `.indices`, int64 on the buffer's device).  An epoch visits them
    in `order` if one is given, under a fresh device permutation (`torch.randperm` from this object's own
    generator) if `shuffle`, as they stand otherwise; `len()` is the number of batches, the last one short unless
    `drop_last`.  Every batch is the reference's 8-tuple after `augment` - state float32 [S*B, 3, R, C], prob
    [S*B, A], winner int8 [S*B, 1], steps_to_end and aux_target int16 [S*B, 1], root_wdl [S*B, 3], valid_mask bool
    [S*B, A], future_root_wdl [S*B, 3], S = 2 (Connect4) or 4 (Othello), rows symmetry-major - in freshly
    allocated tensors (a learner may keep its last batch).

    On a GPU a batch is ONE az_replay_dev_batch on the current stream and nothing waits for the device; the
    permutation is read by the kernel, there is no gather pass.  `route="torch"` is the same thing in plain torch
    (the only route on the CPU, the baseline on a GPU).  Batches read the ring WHEN THEY ARE PRODUCED: an `export`
    between two batches changes what the later ones see (the reference's `sample` snapshots the rows instead; clone
    the buffer's tensors for that).  Work on one stream is ordered, so no row is ever read half written."""

    def __init__(self, buffer, indices, batch_size, order=None, drop_last=False, route=None, shuffle=False, seed=0):
        self.buffer = buffer
        self.game = buffer.game
        dev = buffer.state.device
        self.device = dev
        self.batch_size = int(batch_size)
        if self.batch_size <= 0:
            raise ValueError("batch_size must be positive")
        self.drop_last = bool(drop_last)
        if route is None:
            route = "kernel" if dev.type == "cuda" else "torch"
        if route not in ("kernel", "torch"):
            raise ValueError("route must be 'kernel' or 'torch'")
        if route == "kernel" and dev.type != "cuda":
            raise ValueError("route='kernel' needs the buffer on a GPU")
        self.route = route
        self.indices = torch.as_tensor(indices, dtype=torch.int64).to(dev).contiguous().reshape(-1)
        n = self.indices.numel()
        if order is not None:
            order = torch.as_tensor(order, dtype=torch.int64).contiguous().reshape(-1)
            # host data is checked; a tensor already on the GPU is the caller's word (checking it would wait for the device)
            if order.numel() != n or (n and not order.is_cuda and (int(order.min()) < 0 or int(order.max()) >= n)):
                raise ValueError("order must hold %d positions in [0, %d)" % (n, n))
            order = order.to(dev)
        self.order = order
        self.shuffle = bool(shuffle) and order is None
        if self.shuffle:
            self.gen = torch.Generator(device=dev)
            self.gen.manual_seed(_seed63(seed, 0x45504F43))
        self.S = 2 if self.game == "Connect4" else 4

    def __len__(self):
        n, b = self.indices.numel(), self.batch_size
        return n // b if self.drop_last else (n + b - 1) // b

    def __iter__(self):
        n, b = self.indices.numel(), self.batch_size
        order = torch.randperm(n, device=self.device, generator=self.gen) if self.shuffle else self.order
        src = replay_tensors_c(self.buffer, self.game, self.device, "batches") if self.route == "kernel" else None
        for k in range(len(self)):
            first = k * b
            size = min(b, n - first)
            if self.route == "kernel":
                yield self._kernel_batch(src, order, first, size)
            else:
                at = self.indices[first:first + size] if order is None else self.indices[order[first:first + size]]
                yield self._torch_batch(at)

    def _torch_batch(self, rows):
        buf = self.buffer
        state, prob, mask = _augment_torch(self.game, buf.state[rows].float(), buf.prob[rows], buf.valid_mask[rows])
        rest = [getattr(buf, n)[rows].repeat(self.S, 1) for n in ("winner", "steps_to_end", "aux_target", "root_wdl",
                                                                   "future_root_wdl")]
        return (state, prob, rest[0], rest[1], rest[2], rest[3], mask, rest[4])

    def _kernel_batch(self, src, order, first, size):
        A, R, Cc = REPLAY_GEOMETRY[self.game]
        n = self.S * size
        z = dict(device=self.device)
        out = (torch.empty((n, 3, R, Cc), dtype=torch.float32, **z), torch.empty((n, A), dtype=torch.float32, **z),
               torch.empty((n, 1), dtype=torch.int8, **z), torch.empty((n, 1), dtype=torch.int16, **z),
               torch.empty((n, 1), dtype=torch.int16, **z), torch.empty((n, 3), dtype=torch.float32, **z),
               torch.empty((n, A), dtype=torch.bool, **z), torch.empty((n, 3), dtype=torch.float32, **z))
        c_out = ReplayBatchC(*(t.data_ptr() for t in out))
        with torch.cuda.device(self.device):
            check(lib().az_replay_dev_batch(0 if self.game == "Connect4" else 1, C.byref(src), self.indices.data_ptr(),
                                            None if order is None else order.data_ptr(), first, size,
                                            C.byref(c_out), _stream()))
        return out


class SampledReplayTensors(ReplayTensors):
    """`ReplayTensors` with the reference's `sample` (ReplayBuffer.py:130-145) - the buffer to hand a training
    step: `net.train_step(buffer.sample(512), augmented, ...)`.  (The plain container has no `sample`: what it
    offers is pinned by its tests.)"""

    def __init__(self, game, capacity, device="cpu"):
        super().__init__(game, capacity, device)
        self.sample_calls = 0

    def sample(self, batch_size, full_batches=False, replay_ratio=0.25, seed=0):
        """A sample of the rows stored so far, sized as the reference sizes it (`sample_size`), as `ReplayBatches`
        that reshuffle every epoch; `full_batches` drops the short last batch.  The indices are uniform in
        [0, len(self)): from az_replay_dev_sample_indices on a GPU - keyed by (seed, number of `sample` calls so
        far), enqueued on the current stream, no wait - and from a torch.Generator seeded alike on the CPU."""
        total = len(self)
        assert total > 0
        n = sample_size(total, batch_size, full_batches, replay_ratio)
        call = self.sample_calls
        self.sample_calls += 1
        if self.device.type == "cuda":
            idx = torch.empty(n, dtype=torch.int64, device=self.device)
            with torch.cuda.device(self.device):
                check(lib().az_replay_dev_sample_indices(int(seed) & (2 ** 64 - 1), call, total, idx.data_ptr(), n, _stream()))
        else:
            gen = torch.Generator()
            gen.manual_seed(_seed63(seed, call))
            idx = torch.randint(0, total, (n,), dtype=torch.int64, generator=gen)
        return ReplayBatches(self, idx, batch_size, drop_last=full_batches, shuffle=True, seed=_seed63(seed, call))
