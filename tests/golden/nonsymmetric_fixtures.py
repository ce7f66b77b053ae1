"""Known-answer fixtures for the exponential and the power cone, typed in from the reference's own
tests (data and expected values only), as tests/golden/reference_fixtures.py does for the symmetric
cones.  Each returns (P, q, A, b, cones, expected); the reference checks at atol = 1e-3."""
import numpy as np
import scipy.sparse as sp

from cuclarabel_amd.cones import ZeroConeT, NonnegativeConeT, ExponentialConeT, PowerConeT

ATOL = 1e-3          # test/OptTests/basic_exp.jl:41, basic_pow.jl:43


def basic_exp():
    # test/OptTests/basic_exp.jl:6-34 ; expected :51-62
    n = 7
    A1 = np.hstack([np.ones((1, 3)), np.zeros((1, 4))])
    A2 = np.hstack([np.zeros((3, 2)), -np.eye(3), np.zeros((3, 2))])
    A3 = np.zeros((3, n))
    A3[0, 0] = A3[1, 2] = A3[2, 4] = -1.0
    c = np.array([1.0, 0.5, -2.0, -0.1, 1.0, 3.0, 0.0])
    P = sp.identity(n, format="csc") * 1e-1
    A = sp.csc_matrix(np.vstack([A1, A2, A3]))
    b = np.concatenate([[10.0], np.zeros(3), np.zeros(3)])
    cones = [ZeroConeT(1), NonnegativeConeT(3), ExponentialConeT()]
    x = np.array([-9.425995201329599, 4.828561507482018, 14.59743362204262, 1.0000012112102774,
                  7.65314081561849, -29.99999978458479, -0.0])
    return P, c, A, b, cones, dict(status="SOLVED", x=x, obj=-54.41243965302268)


def basic_pow():
    # test/OptTests/basic_pow.jl:6-36 ; expected :53-54 (status and primal cost only)
    n = 6
    P = sp.csc_matrix((n, n))
    q = np.zeros(n)
    q[2] = q[5] = -1.0
    A = -sp.csc_matrix(np.vstack([np.eye(6), [[1.0, 2.0, 0.0, 3.0, 0.0, 0.0]], [[0.0, 0.0, 0.0, 0.0, 1.0, 0.0]]]))
    b = np.concatenate([np.zeros(6), [-3.0], [-1.0]])
    cones = [PowerConeT(0.6), PowerConeT(0.1), ZeroConeT(1), ZeroConeT(1)]
    return P, q, A, b, cones, dict(status="SOLVED", x=None, obj=-1.8458)
