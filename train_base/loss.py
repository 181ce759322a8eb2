"""Namespace tools/train_stand.py:73-75 does getattr() on: `getattr(loss, name)(**args)`.

Every factory returns a callable usable stand-alone through autograd (HIP kernels underneath) that ALSO carries
`.cruse_loss = (engine loss name, kwargs)`: train.trainer_casual.Trainer reads it to select the fused loss of
cruse_amd.engine.TrainEngine, so `[loss_function] name/args` of the TOML is honoured.  l1_loss / mse_loss keep the
reference's aliases (train_base/loss.py:3-4): the Trainer recognises the torch.nn.L1Loss / MSELoss instance and runs the
fused waveform form (engine losses "l1" / "mse": iSTFT(mask * N) against the clean clip, reduction "mean")."""
import torch

l1_loss = torch.nn.L1Loss
mse_loss = torch.nn.MSELoss


def wo_male_loss(alpha=2.0, beta=1.0):
    """WO-MALE (loss_func/loss.py:121-148) fused with the mask application."""
    from cruse_amd.loss import masked_wo_male

    def fn(mask, noisy_real, noisy_imag, clean_mag):
        return masked_wo_male(mask, noisy_real, noisy_imag, clean_mag, alpha, beta)
    fn.cruse_loss = ("wo_male", dict(loss_alpha=float(alpha), loss_beta=float(beta)))
    return fn


def wo_male_df_loss(alpha=2.0, beta=1.0):
    """WO-MALE on the output of the DeepFilter(1, 5) head (BASELINE config 4): unet_2's output is the real part of the filter
    field, the estimate the 3 x 11 neighbourhood sum of mask * N.  Training runs through the engine (its tag below); stand-alone,
    fn(mask [B,1,T,Fn], noisy [B,2,T,Fs], clean [B,2,T,Fs]) gives the loss VALUE only: the head's inference kernel has no backward."""
    from cruse_amd.loss import deepfilter_spectrum
    from cruse_amd.loss_func import wo_male

    def fn(mask, noisy_spec, clean_spec):
        est = deepfilter_spectrum(mask, noisy_spec[:, 0], noisy_spec[:, 1], 1, 5).permute(0, 3, 1, 2)      # -> [B,2,T,Fs]
        return wo_male(clean_spec, est.contiguous(), noisy_spec, alpha, beta)
    fn.cruse_loss = ("wo_male_df", dict(loss_alpha=float(alpha), loss_beta=float(beta)))
    return fn


def si_snr_loss():
    """train_base/loss.py:7-25 on the HIP path (the engine runs it through the iSTFT on the enhanced waveform)."""
    from cruse_amd.loss import si_snr_loss as _f
    fn = _f()
    fn.cruse_loss = ("si_snr", {})
    return fn


def sdnr_loss(snr=0.0, beta=20.0):
    """sdnr (loss_func/loss.py:151-175, vad == 1) with the mask as gain; snr / beta in dB."""
    from cruse_amd.loss import masked_sdnr

    def fn(mask, clean_real, clean_imag, noisy_real, noisy_imag):
        return masked_sdnr(mask, clean_real, clean_imag, noisy_real, noisy_imag, snr, beta)
    fn.cruse_loss = ("sdnr", dict(snr_db=float(snr), sdnr_beta_db=float(beta)))
    return fn


def multi_res_spec_loss(n_ffts=(128, 256, 512), gamma=0.3, factor=1.0, f_complex=None):
    """MultResSpecLoss (test/test_loss.py:193-229) on the enhanced waveform: the engine runs it through the iSTFT like si_snr_loss."""
    from cruse_amd import ops
    from cruse_amd.loss import multi_res_spec_loss as _f
    fn = _f(n_ffts, gamma, factor, f_complex)
    ns, g, f, fc = ops.mrspec_args(n_ffts, gamma, factor, f_complex)
    fn.cruse_loss = ("mrspec", dict(mrs_ffts=ns, mrs_gamma=g, mrs_factor=f, mrs_f_complex=fc))
    return fn
