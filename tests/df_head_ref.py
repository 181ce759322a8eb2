"""numpy float64 restatement of cruse_df_head_apply (csrc/df_head.hip): the DeepFilter(t_dim, f_dim) head of BASELINE config 4 applied
to the one real filter channel unet_2 emits.

    P[b,t,f] = mask[b,t,f] * N[b,t,f]   for f < Fn,     0 for Fn <= f < Fs,     0 outside [0,T) x [0,Fs)
    E[b,t,f] = sum_{dt=-t_dim..t_dim} sum_{df=-f_dim..f_dim} P[b,t+dt,f+df]     (real and imaginary plane separately)
"""
import numpy as np

# The shapes every test of the head walks: (T, Fs, Fn, t_dim, f_dim).  161 / 160 is the product's spectrum; T runs below, at and above
# the kernel's frame tile (16) and past two tiles; (0,0) is the bare product, (2,5) and (1,0) leave the (1,5) instance; 9 / 8 and
# 6 / 6 have a window wider than the axis; 200 / 199 needs two bin tiles (192).
DIMS = ((1, 5), (0, 0), (2, 5), (1, 0))
CASES = [(T, 161, 160, td, fd) for T in (1, 2, 3, 15, 16, 17, 33) for td, fd in DIMS]
CASES += [(2, 9, 8, 1, 5), (2, 6, 6, 1, 5), (3, 200, 199, 1, 5), (3, 200, 199, 8, 16)]
# the degenerate ones (host test against the oracle's DeepFilter)
DEGENERATE = [(1, 161, 160, 1, 5), (2, 9, 8, 1, 5), (2, 6, 6, 1, 5), (1, 1, 1, 1, 5), (3, 161, 160, 0, 0), (2, 161, 160, 1, 0)]
B = 2


def case_data(T, Fs, Fn, seed=0, batch=B):
    """seeded inputs of one case: mask in (0,1) [batch*T, Fn], normal spectra [batch, T, Fs] (float32)"""
    rng = np.random.default_rng(1000 * seed + 7 * T + Fs)
    mask = (1.0 / (1.0 + np.exp(-rng.standard_normal((batch * T, Fn))))).astype(np.float32)
    nre = rng.standard_normal((batch, T, Fs)).astype(np.float32)
    nim = rng.standard_normal((batch, T, Fs)).astype(np.float32)
    return mask, nre, nim


def df_head(mask, nre, nim, t_dim=1, f_dim=5):
    """mask [B*T, Fn] (or any shape with that many elements), nre / nim [B,T,Fs] -> (ere, eim) float64 [B,T,Fs]"""
    nre, nim = np.asarray(nre, dtype=np.float64), np.asarray(nim, dtype=np.float64)
    Bn, T, Fs = nre.shape
    m = np.asarray(mask, dtype=np.float64).reshape(Bn, T, -1)
    Fn = m.shape[-1]
    assert Fn <= Fs
    out = []
    for plane in (nre, nim):
        P = np.zeros((Bn, T + 2 * t_dim, Fs + 2 * f_dim))
        P[:, t_dim:t_dim + T, f_dim:f_dim + Fn] = m * plane[:, :, :Fn]
        E = np.zeros((Bn, T, Fs))
        for dt in range(2 * t_dim + 1):
            for df in range(2 * f_dim + 1):
                E += P[:, dt:dt + T, df:df + Fs]
        out.append(E)
    return out[0], out[1]
