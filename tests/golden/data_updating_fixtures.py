"""The data of the reference's data-updating tests (test/OptTests/data_updating.jl:6-21 and the ten cases :32-263), typed
in: data and the updates only.  Positions are ZERO-based here (the reference's are one-based): triu(P) stores
[P00, P01, P11], A = [-I; I] stores [A00, A20, A11, A31]."""
import numpy as np
import scipy.sparse as sp

from cuclarabel_amd.cones import NonnegativeConeT

TOL = 1e-7          # data_updating.jl:28


def updating_test_data():
    # data_updating.jl:6-21
    P = sp.csc_matrix(np.array([[4.0, 1.0], [1.0, 2.0]]))
    q = np.array([1.0, 1.0])
    A0 = np.eye(2)
    l, u = np.array([-1.0, -1.0]), np.array([1.0, 1.0])
    A = sp.csc_matrix(np.vstack([-A0, A0]))
    b = np.concatenate([-l, u])
    return P, q, A, b, [NonnegativeConeT(2), NonnegativeConeT(2)]


def _P2():
    return sp.csc_matrix(np.array([[100.0, 1.0], [1.0, 2.0]]))                  # :40-41


def _A2():
    A = updating_test_data()[2].tolil()
    A[1, 1] = -1000.0                                                           # :109-110
    return sp.csc_matrix(A)


# name -> (which of P, q, A, b changes, the update as DeviceSolver takes it, the new value of that datum for a fresh solver)
CASES = {
    "P_matrix": ("P", lambda: sp.triu(_P2(), format="csc"), _P2),                                            # :32-53
    "P_vector": ("P", lambda: sp.triu(_P2(), format="csc").data.copy(), _P2),                                # :55-76
    "P_tuple": ("P", lambda: (np.array([1, 2]), np.array([3.0, 5.0])),
                lambda: sp.csc_matrix(np.array([[4.0, 3.0], [3.0, 5.0]]))),                                   # :78-99 (triu [4 3; 0 5])
    "A_matrix": ("A", _A2, _A2),                                                                             # :101-122
    "A_vector": ("A", lambda: _A2().data.copy(), _A2),                                                       # :124-145
    "A_tuple": ("A", lambda: (np.array([1, 2]), np.array([0.5, -0.5])),
                lambda: sp.csc_matrix(np.array([[-1.0, 0.0], [0.0, -0.5], [0.5, 0.0], [0.0, 1.0]]))),         # :147-169
    "q_vector": ("q", lambda: np.array([10.0, 1.0]), lambda: np.array([10.0, 1.0])),                         # :171-192
    "q_tuple": ("q", lambda: (np.array([1]), np.array([10.0])), lambda: np.array([1.0, 10.0])),              # :194-216
    "b_vector": ("b", lambda: np.zeros(4), lambda: np.zeros(4)),                                             # :218-239
    "b_tuple": ("b", lambda: (np.array([1, 3]), np.array([0.0, 0.0])), lambda: np.array([1.0, 0.0, 1.0, 0.0])),   # :241-263
}
