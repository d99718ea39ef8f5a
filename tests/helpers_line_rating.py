"""Helpers of the line-rating tests (DOPF_F_LINE_RATING), CPU and GPU: the cases and the table the tests share, the
T = 1 column problems the oracle solves with one f_max per line (a column of the table is a problem of its own when no storage
couples the timesteps), and Psi_{n,t} under a rating table for the storages' optimality certificate."""
import copy
import ctypes as C

import numpy as np

from decentralopf_jl_amd import _capi, synth

LR = getattr(_capi, "F_LINE_RATING", 0)
NET = dict(N=4, L=5, seed=50, fmax_factor=0.7, fmax_min=5)
NETC = dict(n_gen=200, n_sto=40, T=24, **NET)                   # the chains' case
GENC = dict(n_gen=40, n_sto=0, T=4, **NET)                      # generators only: every column is a problem of its own
STOC = dict(n_gen=24, n_sto=8, T=12, seed=823, N=4, L=5, fmax_factor=0.7, fmax_min=5)   # storages couple the columns
GAMMA = 0.03


def draw_table(pp, seed=3):
    """f_max scaled per line and timestep by 0.3, 0.6, 1 or 1.5, (L, T)"""
    return pp.f_max[:, None] * np.random.default_rng(seed).choice([0.3, 0.6, 1.0, 1.5], (pp.L, pp.T))


def constant_table(pp, factor=1.0):
    return np.repeat((factor * pp.f_max)[:, None], pp.T, axis=1)


def with_f_max(pp, f_max):
    """the same case with other line limits (one per line)"""
    q = copy.copy(pp)
    q.f_max = np.asarray(f_max, dtype=np.float64).copy()
    return q


def column_problem(pp, t, f_max):
    """the T = 1 problem of timestep t (cases without storages): demand[:, t] and the given limits"""
    assert pp.S == 0
    q = with_f_max(pp, f_max)
    q.T = 1
    q.demand = np.asarray(pp.demand, dtype=np.float64)[:, t:t + 1].copy()
    return q


def rated_engine(api, pp, flags=0, rating=None, **params):
    """a context with the flag; rating: the table set after create (None: the setter is not called)"""
    e = _capi.Engine(api, params=_capi.default_params(flags=flags | LR, **params), **pp.engine_kwargs())
    if rating is not None:
        e.set_line_rating(rating)
    return e


def quiet_state(api, e):
    """dopf_debug_quiet: (the quiet chain is allowed, in use for the next call, times it parked itself)"""
    q = (C.c_int64 * 3)()
    assert api.lib.dopf_debug_quiet(e._ctx, q) == 0
    return int(q[0]), int(q[1]), int(q[2])


def debug_table(api, e, n, t):
    """dopf_debug_table(n, t): beta, psi (2L each), slope (2L + 1), psi0, m"""
    L2 = 2 * e.L
    beta, psi, slope, psi0 = np.zeros(L2), np.zeros(L2), np.zeros(L2 + 1), np.zeros(1)
    m = C.c_int32(0)
    dp = _capi.c_double_p
    rc = api.lib.dopf_debug_table(e._ctx, C.c_int32(n), C.c_int32(t), beta.ctypes.data_as(dp), psi.ctypes.data_as(dp),
                                  slope.ctypes.data_as(dp), psi0.ctypes.data_as(dp), C.byref(m))
    assert rc == 0, rc
    k = int(m.value)
    return dict(beta=beta[:k], psi=psi[:k], slope=slope[:k + 1], psi0=psi0, m=np.asarray([k]))


def psi_at_rated(pp, lam, mu, rho, inj, flow, avg_U, avg_K, gamma, w_flow, dlt, F):
    """helpers_efficiency.psi_at with the line limits per timestep: F is the (L, T) table instead of pp.f_max[None, :, None].
        Psi = pi + gamma (s + dlt) + sum_l w2 h_l [(f + h_l dlt + U_l - F_lt) - (K_l - f - h_l dlt - F_lt)],
        U_l = max(0, (gamma a_l - w2 (f_l + h_l dlt - F_lt)) / (w2 + gamma)),  K_l = max(0, (gamma b_l + w2 (f_l + h_l dlt + F_lt)) / (w2 + gamma))"""
    w2 = 2.0 * w_flow
    h = np.asarray(pp.ptdf, dtype=np.float64).reshape(pp.L, pp.N)[:, np.asarray(pp.sto_node, dtype=np.int64)]      # (L, S)
    psi = lam[None, :] + gamma * (inj.sum(axis=0)[None, :] + dlt)
    if pp.L > 0:
        psi = psi + h.T @ (mu - rho)
        fl = flow[None, :, :] + h.T[:, :, None] * dlt[:, None, :]                    # (S, L, T)
        F = np.asarray(F, dtype=np.float64).reshape(pp.L, pp.T)[None, :, :]
        U = np.maximum(0.0, (gamma * avg_U[None] - w2 * (fl - F)) / (w2 + gamma))
        K = np.maximum(0.0, (gamma * avg_K[None] + w2 * (fl + F)) / (w2 + gamma))
        psi = psi + w2 * np.einsum("ls,slt->st", h, (fl + U - F) - (K - fl - F))
    return psi


def theta_of_rated(pp, before, duals, D, C, gamma, w_flow, F):
    """helpers_efficiency.theta_of under the table F: Psi at the solution's injection change minus gamma (D - C)"""
    q = D - C
    dlt = q - (before["D"] - before["C"])
    flow = np.asarray(pp.ptdf, dtype=np.float64).reshape(pp.L, pp.N) @ before["inj"]
    psi = psi_at_rated(pp, duals[0], duals[1], duals[2], before["inj"], flow, before["avg_U"], before["avg_K"], gamma, w_flow, dlt, F)
    return psi - gamma * q


def case(kw):
    return synth.synthetic_case(**kw)
