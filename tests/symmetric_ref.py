"""numpy restatement of the symmetric bilinear form Qs(g,f) = Q(g,f) + Q(f,g) of include/bfsm.h (test infrastructure).

Two evaluations of tests/bilinear_ref.py on the FULL rule: no antipodal merge, no Hermitian shortcut, whatever the handle under
test does.  antipodal_rule builds the rules on which BFSM_FLAG_EXACT_REDUCTIONS merges directions; wrong_merged is what one
merged pass WITHOUT the exchanged product computes, the operator the tests must be able to tell from the right one.
"""
import numpy as np

import bilinear_ref as BR


def collide_symmetric(g, f, gl, sph, gamma, b_gamma, L, dir_range=None, with_loss=True):
    """Qs(g,f); dir_range = (b0, b1): the symmetric gain of that shard of full directions only."""
    return (BR.collide_bilinear(g, f, gl, sph, gamma, b_gamma, L, dir_range, with_loss) +
            BR.collide_bilinear(f, g, gl, sph, gamma, b_gamma, L, dir_range, with_loss))


def antipodal_rule(n_half, seed=7):
    """random_rule(n_half) followed by its bit-exact negation with the same weights (2 n_half points, weights summing to
    4 pi): the symmetry make_plan verifies before it merges pairs."""
    x, y, z, w = BR.random_rule(n_half, seed)
    w = w / 2
    return np.concatenate([x, -x]), np.concatenate([y, -y]), np.concatenate([z, -z]), np.concatenate([w, w])


def half_rule_doubled(sph):
    """The first half of an antipodal rule with doubled weights: the merged plan's directions."""
    x, y, z, w = sph
    h = len(w) // 2
    return x[:h].copy(), y[:h].copy(), z[:h].copy(), 2 * w[:h]


def wrong_merged(g, f, gl, sph, gamma, b_gamma, L):
    """2 x Q(g,f) on the half rule with doubled weights: a single merged gain pass, the exchanged product left out."""
    return 2 * BR.collide_bilinear(g, f, gl, half_rule_doubled(sph), gamma, b_gamma, L)
