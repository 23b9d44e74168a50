"""torch.optim.SGD's update (momentum, weight decay; no dampening, no nesterov) in float64, with element-wise bounds on
what an fp32 implementation of it may give.

    m1 = mu m0 + g + wd p0          p1 = p0 - lr m1

With S = |g| + |wd p0| + |mu m0|: the buffer takes at most four fp32 roundings (wd p0, g + ., mu m0, the sum -- three
where a product is contracted into an FMA), each of a quantity no larger than S, hence at most 4 x 2^-24 S away; the
parameter inherits that error times |lr| and takes two more roundings (lr m1, the difference), of quantities no larger
than |p0| + |lr| S.  The bounds are twice that count:

    tol_m = 8 x 2^-24 S             tol_p = 8 x 2^-24 (|p0| + |lr| S)
"""
import numpy as np

EPS = 2.0 ** -24
UNITS = 8.0


def expected(p0, m0, g, lr, mu, wd):
    """fp32 arrays p0, m0, g (any shape) and the step's three hyper-parameters (scalars, or arrays that broadcast: one
    value per step) -> (m1, p1, tol_m, tol_p), float64."""
    p0, m0, g, lr, mu, wd = (np.asarray(a, np.float64) for a in (p0, m0, g, lr, mu, wd))
    S = np.abs(g) + np.abs(wd * p0) + np.abs(mu * m0)
    m1 = mu * m0 + g + wd * p0
    p1 = p0 - lr * m1
    return m1, p1, UNITS * EPS * S, UNITS * EPS * (np.abs(p0) + np.abs(lr) * S)
