"""Test tooling: a capture sampled at the 3GPP rate (N = 512 / 1024 / 1536 / 2048 samples per OFDM symbol at 25 / 50 / 75 / 100 PRB) rewritten at
srsRAN's rate (N_r = 384 / 768 / 1024 / 1536), symbol by symbol, in float64.

Per OFDM symbol: take the N useful samples, fft at N, keep the N_r bins around DC (0 .. N_r/2 - 1 and -N_r/2 .. -1), ifft at N_r, prepend the cyclic
prefix of the new length (the last cp_r samples of the new symbol).  The N_r-point DFT of the result EQUALS the N-point DFT of the input on every kept
bin, noise included (numpy's ifft divides by N_r and the receiver's forward transform does not scale), so the receiver at the lower rate sees on the
occupied carriers the values the receiver at the 3GPP rate saw, up to the rounding of the two transforms.

Exact when the capture's symbol timing offset is zero and the channel's delay spread stays inside the cyclic prefix (every symbol is then a circular
convolution, which survives the change of rate); a carrier offset is not band-limited to the kept bins and leaks, as it does in a real resampler.

The uplink antenna carries the half-carrier (7.5 kHz) shift of SC-FDMA: remove it at N (multiply sample n of the useful part by exp(-j pi n / N)),
convert, and put it back at N_r (exp(+j pi n / N_r)).  A PRACH occasion is converted over its own window: 3168 N / 2048 samples of cyclic prefix, then
12 N samples of sequence - use convert_prach_subframe for such a subframe (it must not carry PUSCH as well)."""
import numpy as np

SYMBOL_SZ_3GPP = {6: 128, 15: 256, 25: 512, 50: 1024, 75: 1536, 100: 2048}
SYMBOL_SZ_SRSRAN = {6: 128, 15: 256, 25: 384, 50: 768, 75: 1024, 100: 1536}


def symbol_starts(N, cp):
    """-> [(first sample of the cyclic prefix, cp length)] of the 14 (normal) / 12 (extended CP) symbols of a subframe of 15 N samples"""
    out, pos = [], 0
    for l in range(12 if cp else 14):
        c = N // 4 if cp else (160 if l % 7 == 0 else 144) * N // 2048
        out.append((pos, c))
        pos += c + N
    assert pos == 15 * N
    return out


def _keep(X, Nr):
    """the Nr bins around DC of a spectrum in fft order (last axis)"""
    h = Nr // 2
    return np.concatenate([X[..., :h], X[..., X.shape[-1] - h:]], axis=-1)


def convert_symbol(x, Nr, uplink=False):
    """x[..., N] useful samples of one symbol -> [..., Nr] (complex128); amplitude per carrier preserved in the DFT (see convert_subframes)"""
    x = np.asarray(x, dtype=np.complex128)
    N = x.shape[-1]
    if uplink:
        x = x * np.exp(-1j * np.pi * np.arange(N) / N)
    y = np.fft.ifft(_keep(np.fft.fft(x, axis=-1), Nr), axis=-1)  # DFT_Nr(y) = kept bins of DFT_N(x)
    if uplink:
        y = y * np.exp(1j * np.pi * np.arange(Nr) / Nr)
    return y


def convert_subframes(iq, nof_prb, cp=0, uplink_antennas=(), dtype=np.complex64):
    """iq[..., 15 N] (any leading axes; the axis in front of the samples is the antenna when uplink_antennas is given) at the 3GPP rate ->
    [..., 15 N_r] at srsRAN's rate.  The N_r-point DFT of every converted symbol EQUALS the N-point DFT of the original one on the kept bins (ifft's
    1 / N_r is the whole scaling), so grids, and with them every decision behind them, are comparable value by value."""
    N, Nr = SYMBOL_SZ_3GPP[nof_prb], SYMBOL_SZ_SRSRAN[nof_prb]
    iq = np.asarray(iq)
    assert iq.shape[-1] == 15 * N
    out = np.zeros(iq.shape[:-1] + (15 * Nr,), dtype=np.complex128)
    ul = np.zeros(iq.shape[-2] if iq.ndim >= 2 else 1, dtype=bool)
    for a in uplink_antennas:
        ul[a] = True
    for (p, c), (pr, cr) in zip(symbol_starts(N, cp), symbol_starts(Nr, cp)):
        x = iq[..., p + c:p + c + N]
        y = convert_symbol(x, Nr)
        if ul.any():
            y[..., ul, :] = convert_symbol(x[..., ul, :], Nr, uplink=True)
        out[..., pr + cr:pr + cr + Nr] = y
        out[..., pr:pr + cr] = y[..., Nr - cr:]
    return out.astype(dtype) if dtype is not None else out


def convert_prach_subframe(x, nof_prb, dtype=np.complex64):
    """x[15 N]: an uplink subframe that holds a format-0 PRACH occasion (and no PUSCH) -> [15 N_r].  The detector's window - 3168 N / 2048 samples of
    cyclic prefix, then 12 N samples - is one long symbol: fft at 12 N, the 12 N_r bins around DC, ifft at 12 N_r, the new prefix in front.  What lies
    behind the window (guard time) is left zero; exact for preambles whose delay stays inside the prefix"""
    N, Nr = SYMBOL_SZ_3GPP[nof_prb], SYMBOL_SZ_SRSRAN[nof_prb]
    x = np.asarray(x, dtype=np.complex128)
    assert x.shape[-1] == 15 * N
    cp, cpr = 3168 * N // 2048, 3168 * Nr // 2048
    y = convert_symbol(x[..., cp:cp + 12 * N], 12 * Nr)
    out = np.zeros(x.shape[:-1] + (15 * Nr,), dtype=np.complex128)
    out[..., cpr:cpr + 12 * Nr] = y
    out[..., :cpr] = y[..., 12 * Nr - cpr:]
    return out.astype(dtype) if dtype is not None else out
