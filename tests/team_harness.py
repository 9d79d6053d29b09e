"""Team play - several trees per player and game - restated in numpy for tests that cannot import the reference.

The reference's players search K trees of one root and choose the move from the summed visit counts: root-parallel play
(`AlphaZeroPlayer(n_trees=K)`, src/player.py:248-283) and the symmetry ensemble (`sym_ensemble=True`, player.py:285-329
with src/symmetry.py): tree j is shown the position under the game's j-th symmetry, its visits are mapped back and
summed, the chosen move is mapped into every tree's frame for the re-rooting.  Fixture G21
(tests/golden/make_golden_team.py) holds what the compiled reference and its own Python gave; tests/test_team_cpu.py pins
this restatement to it, the GPU suite compares the native team match (az_match_create_teams) with it.

A team is (trees, ensemble); tree j of game g is tree g * trees + j of that player's search object - the layout of
az_match_create_teams.
"""
import functools

import numpy as np

import match_harness as MH
import scenarios as S

SYM_IDS = {"Connect4": (0, 1), "Othello": (0, 2, 6, 7)}        # symmetry.py:21,46
ACTIONS = {"Connect4": 7, "Othello": 65}
SHAPE = {"Connect4": (6, 7), "Othello": (8, 8)}

# where cell (r, c) of an Othello board goes (symmetry.py:23-32, the four ids in use)
_OT_MOVE = {0: lambda r, c: (r, c), 2: lambda r, c: (7 - r, 7 - c), 6: lambda r, c: (c, r), 7: lambda r, c: (7 - c, 7 - r)}


@functools.lru_cache(maxsize=None)
def cell_perm(game, sym):
    """perm[i] = the cell that cell i (row-major) moves to under `sym` (one shared array per symmetry: read only)."""
    rows, cols = SHAPE[game]
    perm = np.empty(rows * cols, np.intp)
    for i in range(rows * cols):
        r, c = divmod(i, cols)
        nr, nc = (r, cols - 1 - c if sym else c) if game == "Connect4" else _OT_MOVE[sym](r, c)
        perm[i] = nr * cols + nc
    return perm


@functools.lru_cache(maxsize=None)
def action_perm(game, sym):
    """perm[a] = action a under `sym`: Connect4 the column, Othello the square; Othello's pass (64) stays."""
    if game == "Connect4":
        return np.array([6 - a if sym else a for a in range(7)], np.intp)
    return np.append(cell_perm(game, sym), 64)


def sym_board(board, sym, game):
    """symmetry.py:86-95: the board's stones moved by `sym`."""
    board = np.asarray(board)
    out = np.empty(board.size, board.dtype)
    out[cell_perm(game, sym)] = board.ravel()
    return out.reshape(board.shape)


def sym_action(action, sym, game):
    """symmetry.py:98-115 (an involution: the same map both ways); -1 stays."""
    return int(action) if action < 0 else int(action_perm(game, sym)[int(action)])


def inverse_visits(visits, sym, game):
    """symmetry.py:118-137: a tree's visit vector back in the game's frame."""
    visits = np.asarray(visits)
    out = np.empty_like(visits)
    out[action_perm(game, sym)] = visits
    return out


def team_syms(game, team):
    trees, ensemble = team
    if ensemble:
        assert trees == len(SYM_IDS[game])
        return SYM_IDS[game]
    return (0,) * trees


def team_boards(boards, turns, game, team):
    """[n] positions -> the team's roots [n * trees]: every tree its game's position, an ensemble's tree j under symmetry j
    with the side to move as it is (player.py:291-292)."""
    syms = team_syms(game, team)
    out = np.array([sym_board(b, s, game) for b in boards for s in syms], np.int8)
    return out, np.repeat(np.asarray(turns, np.int32), len(syms))


def team_sum(visits, game, team):
    """[n * trees][A] -> [n][A]: every tree's visits mapped back and summed (player.py:299-302, 258-259)."""
    syms = team_syms(game, team)
    v = np.asarray(visits).reshape(-1, len(syms), ACTIONS[game])
    return np.array([sum(inverse_visits(row[j].astype(np.int64), s, game) for j, s in enumerate(syms)) for row in v], np.int64)


def team_actions(actions, game, team):
    """[n] moves of the game's frame -> [n * trees], each in its tree's frame (player.py:321-324)."""
    return np.array([sym_action(a, s, game) for a in actions for s in team_syms(game, team)], np.int32)


def pick(summed, temp, active_idx=None):
    """The move of every game from its summed row: the first most visited action (0 for an empty row: np.argmax of
    zeros, player.py:264-265); with a temperature, pipeline.py:337-351's draw for the active games."""
    summed = np.asarray(summed)
    if temp > 1e-6:
        return MH.sample_actions(summed, temp, range(len(summed)) if active_idx is None else active_idx)
    return np.argmax(summed, axis=1).astype(np.int32)


def action_probs(summed_row):
    """player.py:261-267, 304-310."""
    v = np.asarray(summed_row)
    probs = np.zeros(len(v), np.float32)
    valid = v > 0
    if valid.any():
        probs[valid] = v[valid] / v[valid].sum()
    return probs


def team_decision(w, net, board, turn, game, team, vl_batch=1):
    """One `get_action(env, temp=0)` of a team player (is_selfplay=0: the trees are reset afterwards) on the search
    wrapper `w` of team[0] trees: (raw per-tree visits [trees][A], action, action_probs)."""
    boards, turns = team_boards([board], [turn], game, team)
    w.batch_playout(net, boards, turns, vl_batch=vl_batch)
    raw = np.array(w.get_visits_count(), np.int32)
    summed = team_sum(raw, game, team)[0]
    for i in range(team[0]):
        w.reset_env(i)
    return raw, int(np.argmax(summed)), action_probs(summed)


def team_eval_games(w_p1, w_p2, net_p1, net_p2, Env, n_games, game, teams=((1, False), (1, False)), vl_batch=1, eval_temp=0.0,
                    openings=None, positions=None, fresh_trees=(False, False)):
    """match_harness.batched_eval_games with a team per player: `w_p1` has n_games * teams[0][0] trees, `w_p2`
    n_games * teams[1][0].  The mover's trees get the symmetrised positions, their visits are summed per game, the move
    is picked from the sum, BOTH objects are re-rooted, every tree with the move in its own frame.  Finished games stay
    in the batch and play their arg-max, as there.  Returns winner, length, moves ([plies][n_games], the game's frame)
    and tree_visits (per ply the mover's raw [n_games * trees][A])."""
    envs = MH.start_envs(Env, n_games, openings, positions)
    ws, nets = (w_p1, w_p2), (net_p1, net_p2)
    for w, team in zip(ws, teams):
        for i in range(n_games * team[0]):
            w.reset_env(i)
    done = np.array([bool(e.done()) for e in envs])
    results = np.array([int(e.winPlayer()) if d else 0 for e, d in zip(envs, done)], dtype=np.int32)
    length = np.zeros(n_games, dtype=np.int32)
    moves, tree_visits = [], []
    while not done.all():
        active_idx = np.where(~done)[0]
        current_turn = int(envs[active_idx[0]].turn)
        assert all(int(envs[i].turn) == current_turn for i in active_idx), "one side to move per ply"
        m = 0 if current_turn == 1 else 1
        boards = [np.asarray(e.board).astype(np.int8) for e in envs]
        turns = [int(e.turn) for e in envs]
        if fresh_trees[m]:
            for i in range(n_games * teams[m][0]):
                ws[m].reset_env(i)
        tb, tt = team_boards(boards, turns, game, teams[m])
        ws[m].batch_playout(nets[m], tb, tt, vl_batch=vl_batch)
        raw = np.array(ws[m].get_visits_count(), np.int32)
        tree_visits.append(raw)
        actions = pick(team_sum(raw, game, teams[m]), eval_temp, active_idx)
        for w, team in zip(ws, teams):
            w.prune_roots(team_actions(actions, game, team))
        row = np.full(n_games, -1, np.int32)
        for i in active_idx:
            envs[i].step(int(actions[i]))
            row[i] = actions[i]
            length[i] += 1
            if envs[i].done():
                done[i] = True
                results[i] = envs[i].winPlayer()
        moves.append(row)
    return dict(winner=results, length=length, moves=np.array(moves, np.int32).reshape(len(moves), n_games), tree_visits=tree_visits)


# ---- bitboards (the layout of az_match_set_positions / az_match_team_roots)

def bitboards(boards, game):
    """(bb_p1, bb_p2) uint64 of int8 boards [n][rows][cols]."""
    boards = np.asarray(boards, np.int8)
    return S.boards_to_bitboards(boards) if game == "Connect4" else S.ot_bitboards(boards)


def team_root_bitboards(boards, turns, game, team):
    """What az_match_team_roots must give for these positions: (bb_p1, bb_p2, turns) of n * trees roots."""
    tb, tt = team_boards(boards, turns, game, team)
    b1, b2 = bitboards(tb, game)
    return np.asarray(b1, np.uint64), np.asarray(b2, np.uint64), tt
