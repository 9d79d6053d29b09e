"""Team self-play - several trees per game in the self-play driver - restated in numpy for tests that cannot import the
reference.

The reference's self-play player may search K trees of one root (`AlphaZeroPlayer.get_action` / `_get_action_sym_ensemble`
with is_selfplay=1, src/player.py:248-329): every tree searches the game's position (an ensemble's tree j under symmetry j),
the move and the recorded policy target come from the summed visit counts, every tree is re-rooted with the move mapped
into its own frame.  The team's root statistics are merged by `inverse_sym_stats` (src/symmetry.py:140-186).  Fixture G22
(tests/golden/make_golden_team_stats.py) holds what the compiled reference and its own Python gave; tests/
test_team_selfplay_cpu.py pins this restatement to it, the GPU suite compares the native driver (az_selfplay_create_teams)
and the kernel k_team_root_stats with it.  The symmetry functions and the team layout are tests/team_harness.py's.
"""
import numpy as np

import match_harness as MH
import team_harness as TH

HEAD = ("root_N", "root_Q", "root_M", "root_D", "root_P1W", "root_P2W")
FIELDS = ("N", "Q", "prior", "noise", "M", "D", "P1W", "P2W")
F32 = np.float32


def merged_root_stats(rows, game, team):
    """symmetry.py:140-186 on rows [n * trees][6 + 8A] of root statistics (the layout of get_all_root_stats) -> [n][6 + 8A]:
    float32 throughout, every product and sum rounded on its own, every sum in tree order starting from tree 0's term (what
    numpy does for fewer than 8 trees)."""
    trees = team[0]
    syms = TH.team_syms(game, team)
    A = TH.ACTIONS[game]
    x = np.asarray(rows, F32).reshape(-1, trees, 6 + 8 * A)
    out = np.zeros((x.shape[0], 6 + 8 * A), F32)
    k = F32(trees)

    def seq_sum(terms):
        acc = terms[0].astype(F32).copy()
        for t in terms[1:]:
            acc = (acc + t).astype(F32)
        return acc
    for g, teamrows in enumerate(x):
        out[g, :6] = (seq_sum([r[:6] for r in teamrows]) / k).astype(F32)
        per = [r[6:].reshape(A, 8) for r in teamrows]
        # every column of tree j back in the game's frame
        back = [np.stack([TH.inverse_visits(p[:, q], s, game) for q in range(8)], axis=1) for p, s in zip(per, syms)]
        w = [b[:, 0] for b in back]
        total_w = seq_sum(w)
        o = out[g, 6:].reshape(A, 8)
        o[:, 0] = total_w
        for q in (2, 3):
            o[:, q] = (seq_sum([b[:, q] for b in back]) / k).astype(F32)
        for q in (1, 4, 5, 6, 7):
            num = seq_sum([(b[:, q] * wj).astype(F32) for b, wj in zip(back, w)])
            pos = total_w > 0
            o[pos, q] = (num[pos] / total_w[pos]).astype(F32)
    return out


def stats_rows(w):
    """The wrapper's root statistics as rows [trees][6 + 8A] (get_all_root_stats of its native object)."""
    return np.array(w.mcts.get_all_root_stats(), F32).reshape(w.batch_size, -1)


def action_probs64(summed_row):
    """k_sp_pick's recorded row (player.py:356 as the self-play driver states it): int / int in double, rounded once."""
    v = np.maximum(np.asarray(summed_row, np.int64), 0)
    total = int(v.sum())
    return (v.astype(np.float64) / float(total)).astype(F32) if total > 0 else np.zeros(len(v), F32)


def team_selfplay_ply(w, net, boards, turns, game, team, vl_batch=1):
    """One team search of every game: (raw visits [n * trees][A], summed [n][A], statistics rows [n * trees][6 + 8A])."""
    tb, tt = TH.team_boards(boards, turns, game, team)
    w.batch_playout(net, tb, tt, vl_batch=vl_batch)
    raw = np.array(w.get_visits_count(), np.int32)
    return raw, TH.team_sum(raw, game, team), stats_rows(w)


def team_selfplay_games(w, net, Env, n_games, game, team, vl_batch=1, openings=None, positions=None, tape=None, temp=0.0,
                        epsilons=None, max_plies=None, refill=False):
    """The team self-play loop on the search wrapper `w` of n_games * team[0] trees: per ply team roots, search, summed
    counts, probs, the pick (tape row p while the tape lasts, then the first most visited move; with `temp`,
    MH.sample_actions over the running games), per-tree re-root with the move in each tree's frame, the game step.  A game
    that ends has every tree of its team reset; its slot is dead from then on (action -1 to its trees, no further row) or,
    with `refill`, starts a new game at once.  epsilons(ply) -> the wrapper's noise epsilon of that ply (game.py:87-91).
    Returns `finished`: the games that ended, in the order (finishing ply, slot), each a dict of slot, finish_ply, winner,
    length, the moves, prob rows (float32), merged wdl rows, masks, boards and turns of its plies and the end state as
    bitboards; `running`: the same for the games still in play, per slot; `tree_visits`: per ply the raw per-tree counts."""
    envs = MH.start_envs(Env, n_games, openings, positions)
    for i in range(n_games * team[0]):
        w.reset_env(i)
    dead = np.array([bool(e.done()) for e in envs])
    assert not dead.any()

    def fresh(slot):
        return dict(slot=slot, moves=[], prob=[], wdl=[], mask=[], board=[], turn=[], winner=0, length=0)
    running = [fresh(i) for i in range(n_games)]
    finished, tree_visits, ply = [], [], 0
    while not dead.all() and (max_plies is None or ply < max_plies):
        boards = [np.asarray(e.board).astype(np.int8) for e in envs]
        turns = [int(e.turn) for e in envs]
        if epsilons is not None:
            w.set_noise_epsilon(epsilons(ply))
        raw, summed, stats = team_selfplay_ply(w, net, boards, turns, game, team, vl_batch)
        tree_visits.append(raw)
        merged = merged_root_stats(stats, game, team)
        if tape is not None and ply < len(tape):
            actions = np.asarray(tape[ply], np.int32).copy()
        else:
            actions = TH.pick(summed, temp, np.where(~dead)[0])
        actions[dead] = -1
        w.prune_roots(TH.team_actions(actions, game, team))
        for i in np.where(~dead)[0]:
            if actions[i] < 0:
                continue
            g = running[i]
            g["moves"].append(int(actions[i])); g["prob"].append(action_probs64(summed[i])); g["wdl"].append(merged[i, 3:6].copy())
            g["mask"].append(np.asarray(envs[i].valid_mask(), bool).astype(np.uint8)); g["board"].append(boards[i]); g["turn"].append(turns[i])
            envs[i].step(int(actions[i]))
            g["length"] += 1
            if envs[i].done():
                g["winner"], g["finish_ply"] = int(envs[i].winPlayer()), ply
                g["end"] = tuple(int(v[0]) for v in MH.env_bitboards([envs[i]]))
                finished.append(g)
                for j in range(team[0]):               # the driver resets every tree of a game that ended
                    w.reset_env(i * team[0] + j)
                if refill:
                    envs[i].reset()
                    running[i] = fresh(i)
                else:
                    dead[i] = True
        ply += 1
    return dict(finished=finished, running=running, tree_visits=tree_visits, plies=ply)
