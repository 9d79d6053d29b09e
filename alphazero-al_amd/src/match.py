"""Evaluation matches between two networks on the device: the gate that decides whether a freshly trained
network replaces the best one.

The reference's gate is `TrainPipeline.select_best_player` (src/pipeline.py:241-262) on top of
`_batched_eval_games` (pipeline.py:264-335): two BatchedMCTS objects over the same n games, the side to move
searches in its own, both are re-rooted with every move, moves are drawn from the visit counts at a low
temperature (pipeline.py:337-351) - per-ply Python, numpy sampling per game, Env objects on the host.

`EvaluationMatch` is that loop on the native match driver (az_match_* in include/az_mcts.h): positions, ply
counters, results and the move record live in HBM next to the two engines' trees, and the tail of a ply - the
move, the game step, results, totals - is one kernel (k_match_ply, csrc/match_kernels.hip).  With two native
evaluator models (HIP inference twins, hash evaluators) a step is ONE call into the library (az_match_step);
any other evaluator is searched through `FusedSearch` between az_match_begin_ply and az_match_finish_ply.

Departures from the reference, both deliberate:
  * the reference's two search objects draw Dirichlet noise and symmetry ids from ONE thread-local mt19937
    (MCTS.h:13-17); here each engine has its own device generator stream (seeds `seed` and `seed + 1`), and the
    moves come from a third (keyed by the seed of player +1's engine, the ply and the game);
  * a finished game is not searched again - its slot is dead, both engines' trees of it stay reset; the reference
    goes on searching finished games and discards the move.

`select_best(net, best_net, n_games, threshold)` is pipeline.py:241-262 without the bookkeeping: two halves with
colours swapped, `gate_win_rate` for the arithmetic.

The rating step (`TrainPipeline.update_elo`, pipeline.py:219-239) is here too: `RolloutPlayer` marks a side as the
pure-MCTS rollout player (`MCTSPlayer`, player.py:73-103; searched by k_rollout_search, one launch per search),
`fresh_trees` makes a side start every search from empty trees as `Game.play` does (game.py:41), and
`rating_games(net, ...)` plays the two colour-swapped matches; src/elo.py turns their results into ratings.  Logging
and the best-network bookkeeping stay with the caller.

Teams: the reference's strongest play modes search several trees of one root and choose the move from the summed visit
counts - root-parallel play (`AlphaZeroPlayer(n_trees=K)`, `MCTSPlayer(n_trees=K)`, player.py:73-103, 248-283) and the
symmetry ensemble (`AlphaZeroPlayer(sym_ensemble=True)`, player.py:285-329: one tree per board symmetry, each shown
the position under its symmetry).  `EvaluationMatch(..., n_trees=, sym_ensemble=)` and `RolloutPlayer(n_trees=)` give a
side that many trees per game in its engine; the match driver (az_match_create_teams) spreads the roots, sums the
count rows per game inside the ply's one tail kernel and re-roots every tree with the move in its own frame.

A team's root statistics: `team_root_stats(stats, game, trees, ensemble)` merges the rows of az_mcts_dev_root_stats of every
game's trees into the game's frame as the reference's `inverse_sym_stats` does (src/symmetry.py:140-186, what its GUI shows of
an ensemble search; k_team_root_stats on a GPU tensor, the same arithmetic in torch elsewhere), `root_stats_dict` gives the
reference's dict.  The self-play driver's teams (`NativeSelfPlay(n_trees=, sym_ensemble=)`, src/selfplay.py) record elements
3..5 of it as a ply's root_wdl.
"""
import ctypes as C

import numpy as np
import torch

from src import fused as F
from src.abi import MatchConfig, MatchTeams, lib as match_lib      # noqa: F401  (match_lib: the name callers written before src/abi.py use)
from src.MCTS_cpp import BatchedMCTS
from src.selfplay import _reserve_arenas, _setup_search


def gate_win_rate(results_first, results_second, n_games):
    """pipeline.py:253-256: `results_first` are the winners of the half the candidate played as +1,
    `results_second` of the half it played as -1; a draw counts half.  The denominator is `n_games` as the caller
    asked for them, also when it is odd and only 2 * (n_games // 2) games were played - the reference's figure."""
    first, second = np.asarray(results_first), np.asarray(results_second)
    wins = np.sum(first == 1) + np.sum(second == -1)
    draws = np.sum(first == 0) + np.sum(second == 0)
    return float((wins + 0.5 * draws) / n_games)


def gate_decision(results_first, results_second, n_games, threshold):
    """pipeline.py:256-262 without `update_best_net`: (win_rate >= threshold, win_rate)."""
    rate = gate_win_rate(results_first, results_second, n_games)
    return bool(rate >= threshold), rate


class RolloutPlayer:
    """Marker for `EvaluationMatch`: this side is the reference's pure-MCTS player (`MCTSPlayer`, player.py:73-103) -
    uniform priors, the value of a leaf is the result of a random playout.  Defaults: MCTSPlayer's n_playout and the
    c_puct that `update_elo` passes (pipeline.py:233).  n_trees: root-parallel search (player.py:83,94-101), that many
    independent trees per game, the move from their summed visit counts."""

    def __init__(self, n_playout=1000, c_puct=1.0, n_trees=1):
        self.n_playout, self.c_puct, self.n_trees = int(n_playout), float(c_puct), max(1, int(n_trees))


class _Side:
    """One player's engine and evaluator binding (what selfplay._setup_search builds)."""


def _setup_rollout(self, player, n_trees, seed, game, device):
    """A rollout player's side: an engine only (n_trees trees in all), configured as MCTSPlayer configures it
    (player.py:84-88)."""
    self.B, self.n_playout, self.vl_batch = int(n_trees), player.n_playout, 1
    self.game, self.game_id = game, 0 if game == "Connect4" else 1
    self.MAX_PLIES = 42 if game == "Connect4" else 126
    with torch.cuda.device(device):
        self.search = BatchedMCTS(self.B, c_init=player.c_puct, c_base=500, alpha=0, n_playout=player.n_playout, game_name=game,
                                  noise_epsilon=0.0, fpu_reduction=0.0, use_symmetry=False)
    self.search.seed(seed)
    self.fused = None
    self.h = C.c_void_p(self.search.mcts.handle)
    self.device = device


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


class EvaluationMatch:
    """`n_games` games between `net_p1` (player +1, moves first from the initial position) and `net_p2` (-1).
    Defaults are `_batched_eval_games`'s own: c_base 500, noise epsilon 0.05, temperature 0.2, the wrapper's
    fpu_reduction.  `c_init` may be a pair (player +1, player -1): search parameters live in each engine's own
    config.  positions: (bb_p1, bb_p2, turns) as integer arrays of n_games entries, one side to move throughout -
    an opening suite instead of the initial position.  `play()` runs to the end and returns the winners
    (int32, +1 / -1 / 0) like the reference; `step(n)`, `remaining()`, `results()`, `moves()` are the pieces.
    Either side may be a `RolloutPlayer` (its own n_playout and c_puct; the other arguments configure network sides).
    fresh_trees (a flag or a pair): that side starts every one of its searches from empty trees instead of the
    subtree its re-rooting kept (game.py:41).
    n_trees, sym_ensemble (each a value or a pair): a network side searches n_trees trees per game (root-parallel,
    player.py:248-283) or, as an ensemble, one tree per board symmetry of the game (2 / 4; player.py:285-329) with the
    engine's own random symmetry off (player.py:177-180); a RolloutPlayer brings its own n_trees and is never an
    ensemble.  The side's engine holds n_games * trees trees.  eval_noise_eps may be a pair as well: root-parallel
    trees of a deterministic evaluator differ only through their root noise (player.py:112-117)."""

    def __init__(self, net_p1, net_p2, n_games, n_playout=200, vl_batch=1, c_init=1.25, c_base=500, alpha=0.3,
                 eval_noise_eps=0.05, eval_temp=0.2, use_symmetry=True, mlh_slope=0.0, mlh_cap=0.2,
                 score_utility_factor=0.0, score_scale=8.0, value_decay=1.0, fpu_reduction=0.4, seed=0, game="Connect4",
                 table_log2=0, positions=None, record_moves=False, reserve_slots=None, fresh_trees=False, n_trees=1,
                 sym_ensemble=False):
        self._mt = None
        self.B, self.n_playout, self.vl_batch = int(n_games), int(n_playout), int(vl_batch)
        self.game = game
        self.fresh_trees = sum((1 << i) for i, f in enumerate(_pair(fresh_trees)) if f)
        self.sides = [None, None]
        nets = (net_p1, net_p2)
        n_sym = 2 if game == "Connect4" else 4                # az_game_num_augment
        self.ensemble = tuple(bool(f) and not isinstance(net, RolloutPlayer) for f, net in zip(_pair(sym_ensemble), nets))
        self.trees = tuple(net.n_trees if isinstance(net, RolloutPlayer) else n_sym if ens else max(1, int(k))
                           for net, ens, k in zip(nets, self.ensemble, _pair(n_trees)))
        for i, (net, ci, eps) in enumerate(zip(nets, _pair(c_init), _pair(eval_noise_eps))):
            if isinstance(net, RolloutPlayer):
                continue
            s = _Side()
            _setup_search(s, net, self.B * self.trees[i], n_playout, vl_batch, ci, c_base, alpha, eps, fpu_reduction,
                          use_symmetry and not self.ensemble[i],
                          mlh_slope, mlh_cap, value_decay, eval_temp, 0, eval_temp, int(seed) + i, table_log2, game,
                          score_utility_factor, score_scale)
            self.sides[i] = s
        dev = next((s.device for s in self.sides if s is not None), torch.device("cuda", torch.cuda.current_device()))
        for i, net in enumerate(nets):                        # rollout players go where the network side is
            if self.sides[i] is None:
                self.sides[i] = _Side()
                _setup_rollout(self.sides[i], net, self.B * self.trees[i], int(seed) + i, game, dev)
        for s in self.sides:
            _reserve_arenas(s, reserve_slots)
        self.device = self.sides[0].device
        self.MAX_PLIES = self.sides[0].MAX_PLIES
        self.A = self.sides[0].search.action_size
        self._ones = [None, None]                             # reset masks of the begin / search / finish route
        self.L = F.lib()
        self.config = MatchConfig(float(eval_temp), int(bool(record_moves)))
        self.record_moves = bool(record_moves)
        self.teams = MatchTeams(self.trees[0], self.trees[1], int(self.ensemble[0]), int(self.ensemble[1]))
        mt = C.c_void_p()
        with torch.cuda.device(self.device):
            F.check(self.L.az_match_create_teams(self.sides[0].h, self.sides[1].h, C.byref(self.config), C.byref(self.teams),
                                                 C.byref(mt)))
        self._mt = mt
        self._tape = None
        self.poll_every = 4
        if positions is not None:
            self.set_positions(*positions)

    def __del__(self):
        try:
            if self.__dict__.get("_mt") is not None:          # before the engines it borrows
                mt, self._mt = self._mt, None
                self.L.az_match_destroy(mt)
        except Exception:
            pass

    def set_positions(self, bb_p1, bb_p2, turns):
        a = np.ascontiguousarray(np.asarray(bb_p1).astype(np.uint64))
        b = np.ascontiguousarray(np.asarray(bb_p2).astype(np.uint64))
        t = np.ascontiguousarray(turns, dtype=np.int32)
        assert a.shape == b.shape == t.shape == (self.B,)
        with torch.cuda.device(self.device):
            F.check(self.L.az_match_set_positions(self._mt, a.ctypes.data, b.ctypes.data, t.ctypes.data))

    def set_action_tape(self, actions):
        """actions: (n_plies, n_games) integers, -1 where a game is over; None ends the tape (test hook)."""
        if actions is None:
            self._tape = None
            F.check(self.L.az_match_set_action_tape(self._mt, None, 0))
            return
        t = torch.as_tensor(np.ascontiguousarray(actions, dtype=np.int32)).to(self.device).contiguous()
        assert t.dim() == 2 and t.shape[1] == self.B
        torch.cuda.current_stream().synchronize()
        self._tape = t                                        # read by the kernel: kept alive here
        F.check(self.L.az_match_set_action_tape(self._mt, t.data_ptr(), t.shape[0]))

    def native_models(self):
        """(model of +1, model of -1) when every network side has a native model object (None stands for a rollout
        player's side), else None."""
        models = []
        for s in self.sides:
            if s.fused is None:
                models.append(None)
                continue
            s.fused._sync_fast_net()
            m = s.fused._native_model()
            if m is None:
                return None
            models.append(m)
        return tuple(models)

    def step(self, n=1):
        """n plies in every game that is still running."""
        models = self.native_models()
        s = F._stream()
        nets = [x.fused for x in self.sides if x.fused is not None]
        table = 1 if nets and nets[0].table_log2 else 0
        with torch.cuda.device(self.device):
            if models is not None and (self.fresh_trees or None in models):
                F.check(self.L.az_match_step_players(self._mt, models[0], models[1], self.sides[0].n_playout, self.sides[1].n_playout,
                                                     max(1, self.vl_batch), table, self.fresh_trees, int(n), s))
                return
            if models is not None:
                F.check(self.L.az_match_step(self._mt, models[0], models[1], self.n_playout, max(1, self.vl_batch), table,
                                             int(n), s))
                return
            mover = C.c_int()
            for _ in range(int(n)):
                F.check(self.L.az_match_begin_ply(self._mt, s, C.byref(mover)))
                if mover.value == 0:
                    return
                i = 0 if mover.value > 0 else 1
                side = self.sides[i]
                if (self.fresh_trees >> i) & 1:
                    if self._ones[i] is None:
                        self._ones[i] = torch.ones(side.B, dtype=torch.uint8, device=self.device)
                    F.check(self.L.az_mcts_dev_reset_masked(side.h, self._ones[i].data_ptr(), s))
                if side.fused is None:
                    F.check(self.L.az_mcts_dev_rollout_search(side.h, side.n_playout, 0, s))
                else:
                    side.fused.search(self.n_playout, self.vl_batch)
                F.check(self.L.az_match_finish_ply(self._mt, s))

    def remaining(self):
        """Games still running (synchronises)."""
        n = C.c_int64()
        F.check(self.L.az_match_remaining(self._mt, C.byref(n)))
        return n.value

    def play(self):
        """Every game to its end: the winners, int32 [n_games] (pipeline.py:335).  The host asks how many games
        are left every `poll_every` plies, not every ply, and never plays past the game's ply bound."""
        played = 0
        while played < self.MAX_PLIES:
            n = min(int(self.poll_every), self.MAX_PLIES - played)
            self.step(n)
            played += n
            if self.remaining() == 0:
                break
        return self.results()["winner"]

    def results(self):
        """winner (+1 / -1 / 0; 0 while running) and length per game, totals (synchronises)."""
        w, ln, t = np.zeros(self.B, np.int32), np.zeros(self.B, np.int32), (C.c_int64 * 4)()
        F.check(self.L.az_match_results(self._mt, w.ctypes.data, ln.ctypes.data, C.byref(t)))
        return dict(winner=w, length=ln, p1_wins=t[0], p2_wins=t[1], draws=t[2], running=t[3])

    def moves(self):
        """With record_moves: int32 [max_plies, n_games], -1 where the game had ended (synchronises)."""
        assert self.record_moves
        out = np.zeros((self.MAX_PLIES, self.B), np.int32)
        F.check(self.L.az_match_moves(self._mt, out.ctypes.data))
        return out

    def engine_counters(self):
        return tuple(F.counters(s.h) for s in self.sides)


STAT_HEAD = ("root_N", "root_Q", "root_M", "root_D", "root_P1W", "root_P2W")          # a root-statistics row: the head ...
STAT_FIELDS = ("N", "Q", "prior", "noise", "M", "D", "P1W", "P2W")                      # ... then these per action


def team_action_perms(game, trees, ensemble=False):
    """perm[j][a]: action a of the game's frame in the frame of tree j of a team (csrc/board_sym.h `ensemble_action`;
    involutions, Othello's pass stays); the identity for every tree of a root-parallel team."""
    A = 7 if game == "Connect4" else 65
    perms = np.tile(np.arange(A, dtype=np.int64), (int(trees), 1))
    if ensemble:
        assert int(trees) == (2 if game == "Connect4" else 4), "an ensemble has one tree per symmetry of the game"
        if game == "Connect4":
            perms[1] = 6 - perms[1]
        else:
            r, c = np.arange(64) // 8, np.arange(64) % 8
            perms[1, :64], perms[2, :64], perms[3, :64] = 63 - np.arange(64), c * 8 + r, (7 - c) * 8 + (7 - r)
    return perms


def _team_root_stats_torch(stats, game, trees, ensemble):
    """k_team_root_stats in torch: float32 throughout, every product and sum an operation of its own, sums in tree order."""
    A = 7 if game == "Connect4" else 65
    x = stats.reshape(-1, trees, 6 + 8 * A).to(torch.float32)
    k = torch.tensor(float(trees), dtype=torch.float32, device=x.device)

    def seq_sum(t):                                           # [n, trees, ...] -> [n, ...], tree 0 first
        acc = t[:, 0].clone()
        for j in range(1, trees):
            acc = acc + t[:, j]
        return acc
    perms = torch.as_tensor(team_action_perms(game, trees, ensemble), device=x.device)
    # tree j's row of action a sits at a's index in that tree's frame
    per = x[:, :, 6:].reshape(-1, trees, A, 8)
    per = torch.gather(per, 2, perms[None, :, :, None].expand(per.shape[0], trees, A, 8))
    w = per[..., 0]
    n_sum = seq_sum(w)
    out = torch.zeros((x.shape[0], A, 8), dtype=torch.float32, device=x.device)
    out[..., 0] = n_sum
    for q in (2, 3):
        out[..., q] = seq_sum(per[..., q]) / k
    for q in (1, 4, 5, 6, 7):
        num = seq_sum(per[..., q] * w)
        out[..., q] = torch.where(n_sum > 0, num / n_sum, torch.zeros_like(num))
    return torch.cat([seq_sum(x[:, :, :6]) / k, out.reshape(-1, 8 * A)], dim=1)


def team_root_stats(stats, game, trees, ensemble=False, route=None):
    """The root statistics of teams of trees merged into each game's frame - the reference's `inverse_sym_stats`
    (src/symmetry.py:140-186) for trees j = 0 .. trees - 1 of every game, with the game's ensemble symmetries
    (`ensemble`) or the identity for every tree (a root-parallel team).  stats: float32 tensor [n * trees, 6 + 8A] laid
    out as az_mcts_dev_root_stats writes it (tree j of game g in row g * trees + j); returns [n, 6 + 8A] on the same
    device.  route: "kernel" (az_mcts_dev_team_root_stats, a GPU tensor) or "torch" (the same arithmetic in torch ops);
    None takes the kernel for a GPU tensor and torch for a CPU tensor - the only route there."""
    trees = int(trees)
    A = 7 if game == "Connect4" else 65
    assert game in ("Connect4", "Othello") and trees >= 1
    assert stats.dim() == 2 and stats.shape[1] == 6 + 8 * A and stats.shape[0] % trees == 0 and stats.dtype == torch.float32
    assert not ensemble or trees == (2 if game == "Connect4" else 4), "an ensemble has one tree per symmetry of the game"
    if route is None:
        route = "kernel" if stats.is_cuda else "torch"
    assert route in ("kernel", "torch")
    if route == "torch":
        return _team_root_stats_torch(stats, game, trees, bool(ensemble))
    assert stats.is_cuda, "team_root_stats: the kernel route needs a GPU tensor"
    stats = stats.contiguous()
    n = stats.shape[0] // trees
    merged = torch.empty((n, 6 + 8 * A), dtype=torch.float32, device=stats.device)
    with torch.cuda.device(stats.device):
        F.check(F.lib().az_mcts_dev_team_root_stats(0 if game == "Connect4" else 1, stats.data_ptr(), trees, int(bool(ensemble)),
                                                    merged.data_ptr(), n, F._stream()))
    return merged


def root_stats_dict(merged, A):
    """Rows [n, 6 + 8A] of root statistics as the reference's `get_root_stats` / `inverse_sym_stats` dict: root_N ..
    root_P2W arrays of shape (n,), N .. P2W of shape (n, A); float32 numpy."""
    m = merged.detach().cpu().numpy() if isinstance(merged, torch.Tensor) else np.asarray(merged, np.float32)
    assert m.ndim == 2 and m.shape[1] == 6 + 8 * int(A)
    out = {k: m[:, i].copy() for i, k in enumerate(STAT_HEAD)}
    per = m[:, 6:].reshape(m.shape[0], int(A), 8)
    out.update({k: per[:, :, i].copy() for i, k in enumerate(STAT_FIELDS)})
    return out


def rating_games(net, n_games, n_playout, pure_mcts_n_playout, n_trees=1, sym_ensemble=False, rollout_trees=1, **kw):
    """The games of one rating round (`TrainPipeline.update_elo`, pipeline.py:219-239): `n_games` with `net` as +1
    against the rollout player, then `n_games` with the colours swapped, both sides starting every search from empty
    trees.  Returns (winners with net as +1, winners with net as -1), int32 +1 / -1 / 0 each.  The network side
    searches as `update_elo` configures it - no root noise, the most visited move, c_base 500; other keyword
    arguments go to EvaluationMatch (the second match uses seed + 2).  n_games = 1 is the reference's round; with
    more, the rollout player's randomness makes the games differ.  src/elo.py's `rate` turns the pair into ratings.
    n_trees / sym_ensemble: the network side plays root-parallel or as the symmetry ensemble; rollout_trees: the rollout
    player's trees per game.  Without an eval_noise_eps of the caller's the network side takes what
    `AlphaZeroPlayer.eval()` sets (player.py:221-232): 0.05 when root-parallel, 0 for an ensemble or a single tree."""
    seed = int(kw.pop("seed", 0))
    eps = 0.05 if int(n_trees) > 1 and not sym_ensemble else 0.0
    kw = dict(dict(eval_noise_eps=eps, eval_temp=0.0, c_base=500, fresh_trees=True), **kw)
    rollout = RolloutPlayer(pure_mcts_n_playout, 1.0, rollout_trees)
    first = EvaluationMatch(net, rollout, n_games, n_playout=n_playout, seed=seed, n_trees=n_trees, sym_ensemble=sym_ensemble,
                            **kw).play()
    second = EvaluationMatch(rollout, net, n_games, n_playout=n_playout, seed=seed + 2, n_trees=n_trees,
                             sym_ensemble=sym_ensemble, **kw).play()
    return first, second


def select_best(net, best_net, n_games, threshold, **kw):
    """pipeline.py:241-262: n_games // 2 games with `net` as +1, as many with `best_net` as +1;
    returns (win_rate >= threshold, win_rate).  Keyword arguments go to EvaluationMatch (the second half uses
    seed + 2, its engines' generators differ from the first half's)."""
    n_half = int(n_games) // 2
    seed = int(kw.pop("seed", 0))
    first = EvaluationMatch(net, best_net, n_half, seed=seed, **kw).play() if n_half else np.zeros(0, np.int32)
    second = EvaluationMatch(best_net, net, n_half, seed=seed + 2, **kw).play() if n_half else np.zeros(0, np.int32)
    return gate_decision(first, second, n_games, threshold)
