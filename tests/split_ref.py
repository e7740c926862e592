"""numpy restatement of the gain / loss split of include/bfsm.h (bfsm_collide_split*; test infrastructure).

Built from what tests/bilinear_ref.py already pins to the oracle:
    Qgain = collide_bilinear(g, f, with_loss=False)   -- Re IFFT(Q_gain_hat[g_hat, f_hat]) of the directions asked for
    nu    = loss_rate(f)                              -- Re IFFT(beta2 f_hat / G), the collision frequency
so that Q(g,f) = Qgain - g * nu.  tests/test_emu_split.py pins the assembled Q(f,f) to the oracle.
"""
import bilinear_ref as BR


def split(g, f, gl, sph, gamma, b_gamma, L, dir_range=None):
    """(Qgain, nu) of Q(g,f); g = f gives the split of Q(f,f).  dir_range: the gain of that shard of directions only."""
    Qgain = BR.collide_bilinear(g, f, gl, sph, gamma, b_gamma, L, dir_range=dir_range, with_loss=False)
    return Qgain, BR.loss_rate(f, gl, gamma, b_gamma, L)
