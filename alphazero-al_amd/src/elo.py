"""Elo arithmetic of the rating step (the reference's `Elo`, src/utils.py:8-22, as `TrainPipeline.update_elo` drives
it, pipeline.py:219-239).  Learner-side code: plain Python floats, no engine, no torch - the games come from
`src.match.rating_games`, this module only turns their results into ratings.
"""


class Elo:
    """Two ratings, A (the network) and B (the rollout player).  `update(result_a)` with result_a = 1 (A won), 0.5
    (draw) or 0 (A lost) moves both by k times (score - expected score); neither rating falls below 1500
    (utils.py:20-21)."""

    def __init__(self, init_a=1500, init_b=1500):
        self.R_A = init_a
        self.R_B = init_b

    def update(self, result_a, k=32):
        gap = (self.R_B - self.R_A) / 400             # the logistic curve with base 10 and scale 400
        expect_a, expect_b = 1 / (1 + 10 ** gap), 1 / (1 + 10 ** -gap)
        a = self.R_A + k * (result_a - expect_a)
        b = self.R_B + k * ((1 - result_a) - expect_b)
        self.R_A, self.R_B = max(a, 1500), max(b, 1500)
        return self.R_A, self.R_B


def score(winner, net_side):
    """1 / 0.5 / 0 from the network's side (pipeline.py:236,239): `winner` is +1, -1 or 0, the network played `net_side`."""
    w = int(winner)
    return 0.5 if w == 0 else (1 if w == net_side else 0)


def rate(elo, results_as_p1, results_as_p2, k=32):
    """One `update` per game, in the order first[0], second[0], first[1], second[1], ...: `results_as_p1` are the
    winners of the games the network played as +1, `results_as_p2` of those it played as -1 (what
    `src.match.rating_games` returns).  With one game per colour this is `update_elo`'s sequence; with more it is the
    same rule applied more often - a longer sequence of the reference's updates, not a different estimator.  Returns
    (R_A, R_B) after the last update (the current ratings when there are no games)."""
    first, second = list(results_as_p1), list(results_as_p2)
    for i in range(max(len(first), len(second))):
        if i < len(first):
            elo.update(score(first[i], 1), k)
        if i < len(second):
            elo.update(score(second[i], -1), k)
    return elo.R_A, elo.R_B
