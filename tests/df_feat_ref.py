"""float64 numpy restatement of cruse_df_feat, written from the formulas in include/cruse_hip.h: the sequential loop
along time, no torch.  Also the same formulas in torch float32 on the CPU (the yardstick of the accuracy bar) and the test signals."""
import numpy as np

ERB_INIT = (-60.0, -90.0)
UNIT_INIT = (0.001, 0.0001)


def default_states(B, nb_erb, nb_df):
    return (np.tile(np.linspace(ERB_INIT[0], ERB_INIT[1], nb_erb), (B, 1)) if nb_erb else None,
            np.tile(np.linspace(UNIT_INIT[0], UNIT_INIT[1], nb_df), (B, 1)) if nb_df else None)


def starts_of(widths):
    return np.concatenate([[0], np.cumsum(np.asarray(widths, dtype=np.int64))])


def df_feat(re, im, starts, nb_df, alpha, erb_state=None, unit_state=None, log_eps=1e-10, erb_scale=40.0, unit_eps=1e-14):
    """re, im [B,T,F]; starts: [nb_erb + 1] or None.  -> feat_erb [B,T,nb_erb], feat_spec [B,T,nb_df,2], the two final states (None for
    a feature that is off).  States absent: the defaults."""
    re, im = np.asarray(re, dtype=np.float64), np.asarray(im, dtype=np.float64)
    B, T, F = re.shape
    alpha = float(alpha)
    nb_erb = 0 if starts is None else len(starts) - 1
    d_erb, d_unit = default_states(B, nb_erb, nb_df)
    p = re * re + im * im
    feat_erb = feat_spec = m = s = None
    if nb_erb:
        m = np.array(d_erb if erb_state is None else erb_state, dtype=np.float64)
        feat_erb = np.zeros((B, T, nb_erb))
        for t in range(T):
            e = np.stack([10.0 * np.log10(p[:, t, starts[j]:starts[j + 1]].sum(axis=-1) / (starts[j + 1] - starts[j]) + log_eps)
                          for j in range(nb_erb)], axis=-1)
            m = e * (1.0 - alpha) + alpha * m
            feat_erb[:, t] = (e - m) / erb_scale
    if nb_df:
        s = np.array(d_unit if unit_state is None else unit_state, dtype=np.float64)
        feat_spec = np.zeros((B, T, nb_df, 2))
        for t in range(T):
            a = np.sqrt(np.maximum(p[:, t, :nb_df], unit_eps))
            s = a * (1.0 - alpha) + alpha * s
            q = np.sqrt(s)
            feat_spec[:, t, :, 0] = re[:, t, :nb_df] / q
            feat_spec[:, t, :, 1] = im[:, t, :nb_df] / q
    return feat_erb, feat_spec, m, s


def df_feat_torch32(re, im, starts, nb_df, alpha, erb_state=None, unit_state=None, log_eps=1e-10, erb_scale=40.0, unit_eps=1e-14):
    """The same formulas by torch in float32 on the CPU (ExponentialUnitNorm.forward's own operations for the unit norm): its error against
    the float64 restatement is what the kernel's error is measured by.  -> feat_erb, feat_spec and the two final states."""
    import torch
    re, im = torch.from_numpy(np.array(re, dtype=np.float32)), torch.from_numpy(np.array(im, dtype=np.float32))
    B, T, F = re.shape
    nb_erb = 0 if starts is None else len(starts) - 1
    d_erb, d_unit = default_states(B, nb_erb, nb_df)
    x = torch.stack([re, im], dim=-1)
    p = x.square().sum(dim=-1)
    feat_erb = feat_spec = m_out = s_out = None
    if nb_erb:
        m = torch.tensor(np.asarray(d_erb if erb_state is None else erb_state), dtype=torch.float32)
        e = 10.0 * torch.log10(torch.stack([p[..., starts[j]:starts[j + 1]].mean(dim=-1) for j in range(nb_erb)], dim=-1) + log_eps)
        out = []
        for t in range(T):
            m = e[:, t] * (1 - alpha) + alpha * m
            out.append((e[:, t] - m) / erb_scale)
        feat_erb = torch.stack(out, 1).numpy() if T else np.zeros((B, 0, nb_erb), np.float32)
        m_out = m.numpy()
    if nb_df:
        s = torch.tensor(np.asarray(d_unit if unit_state is None else unit_state), dtype=torch.float32).unsqueeze(-1)
        xd = x[:, :, :nb_df]
        x_abs = xd.square().sum(dim=-1, keepdim=True).clamp_min(unit_eps).sqrt()
        out = []
        for t in range(T):
            s = x_abs[:, t] * (1 - alpha) + s * alpha
            out.append(s)
        feat_spec = (xd / torch.stack(out, 1).sqrt()).numpy() if T else np.zeros((B, 0, nb_df, 2), np.float32)
        s_out = s.squeeze(-1).numpy()
    return feat_erb, feat_spec, m_out, s_out


def spectrum(B, T, F, seed, dbfs=-25.0):
    """A seeded harmonic stack plus noise per clip at about `dbfs`, as its one-sided STFT (Hann, n_fft = 2 (F - 1), hop = n_fft / 2,
    frames taken from the start without padding): re, im float32 [B,T,F]."""
    rng = np.random.default_rng(seed)
    n_fft, hop = 2 * (F - 1) if F > 1 else 2, max(F - 1, 1)
    L = n_fft + hop * max(T - 1, 0)
    t = np.arange(L) / 16000.0
    x = np.zeros((B, L))
    for b in range(B):
        f0 = rng.uniform(90.0, 320.0)
        for h in range(1, 9):
            x[b] += rng.uniform(0.2, 1.0) / h * np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 2 * np.pi))
        x[b] += 0.1 * rng.standard_normal(L)
        x[b] *= 10.0 ** (dbfs / 20.0) / np.sqrt(np.mean(x[b] ** 2))
    win = np.hanning(n_fft + 1)[:-1]
    frames = np.stack([x[:, i * hop:i * hop + n_fft] * win for i in range(T)], axis=1) if T else np.zeros((B, 0, n_fft))
    spec = np.fft.rfft(frames, axis=-1)[..., :F]
    return np.ascontiguousarray(spec.real.astype(np.float32)), np.ascontiguousarray(spec.imag.astype(np.float32))
