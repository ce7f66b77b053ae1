"""Known-answer fixture for the generalized power cone, typed in from the reference's own test (data and expected
values only), as tests/golden/nonsymmetric_fixtures.py does for the exponential and the power cone.  Returns
(P, q, A, b, cones, expected); the reference checks at atol = 1e-3."""
import numpy as np
import scipy.sparse as sp

from cuclarabel_amd.cones import ZeroConeT, GenPowerConeT

ATOL = 1e-3          # test/OptTests/basic_genpow.jl:39


def basic_genpow():
    # test/OptTests/basic_genpow.jl:7-32 ; expected :49-50 (status and primal cost only)
    n = 6
    P = sp.csc_matrix((n, n))
    q = np.zeros(n)
    q[2] = q[5] = -1.0
    A = sp.csc_matrix(np.vstack([-np.eye(6), [[1.0, 2.0, 0.0, 3.0, 0.0, 0.0]], [[0.0, 0.0, 0.0, 0.0, 1.0, 0.0]]]))
    b = np.concatenate([np.zeros(6), [3.0], [1.0]])
    cones = [GenPowerConeT([0.6, 0.4], 1), GenPowerConeT([0.1, 0.9], 1), ZeroConeT(2)]
    return P, q, A, b, cones, dict(status="SOLVED", x=None, obj=-1.8458)
