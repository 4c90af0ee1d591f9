"""Reference of the slot encoding (test helper only): the definition evaluated directly in numpy longdouble, exact rounding, Python
integers for the residues and the oracle's transform for the limbs.

N = ring degree, n = N / 2 slots, zeta = exp(i pi / N), e_j = 5^j mod 2N.
    encode   m_k = (2 / N) Re sum_j z_j zeta^(-e_j k),  k < N;   c_k = rint(Delta m_k), ties to even
    decode   z_j = sum_k m_k zeta^(e_j k),  m_k = c_k / Delta
Every power of zeta is looked up in a table of the 2N roots by its exponent reduced with integers, so no angle is ever larger than 2 pi.
`exact_coeffs` / `exact_slots` are the O(n N) definition, by row blocks; `fft_coeffs` / `fft_slots` the same maps through a radix-2 transform in
longdouble (the host path a caller without the library would use, and the reference at ring sizes where the definition is too slow): its error is
a few 2^-64 per stage, far below anything the double transform under test can resolve; tests/test_slots_ref.py checks it against the definition."""
import numpy as np

LD = np.longdouble


def rot_group(logN):
    N = 1 << logN
    e, out = 1, np.empty(N // 2, dtype=np.int64)
    for j in range(N // 2):
        out[j] = e
        e = e * 5 % (2 * N)
    return out


_roots = {}


def roots(logN):
    """(cos, sin)(pi t / N), t < 2N, in longdouble"""
    if logN not in _roots:
        N = 1 << logN
        ang = np.arccos(LD(-1)) * np.arange(2 * N).astype(LD) / LD(N)
        _roots[logN] = (np.cos(ang), np.sin(ang))
    return _roots[logN]


def exact_coeffs(z, logN, block=256):
    """m_k, k < N, of the slot vector z (complex, length N / 2): the definition, longdouble"""
    N = 1 << logN
    n = N // 2
    z = np.asarray(z)
    assert z.shape == (n,)
    cs, sn = roots(logN)
    e = rot_group(logN)
    nz = np.nonzero(z)[0]   # a term with z_j = 0 adds nothing
    zr, zi, e = z.real.astype(LD)[nz], z.imag.astype(LD)[nz], e[nz]
    m = np.zeros(N, dtype=LD)
    if len(nz) == 0:
        return m
    for k0 in range(0, N, block):
        k = np.arange(k0, min(N, k0 + block), dtype=np.int64)
        t = (-(k[:, None] * e[None, :])) % (2 * N)
        # Re(z zeta^t) = z_re cos - z_im sin
        m[k0:k0 + len(k)] = (cs[t] * zr[None, :] - sn[t] * zi[None, :]).sum(axis=1)
    return m * (LD(2) / LD(N))


def exact_slots(m, logN, block=256):
    """z_j = sum_k m_k zeta^(e_j k) for real m of length N: (re, im) in longdouble"""
    N = 1 << logN
    n = N // 2
    m = np.asarray(m).astype(LD)
    cs, sn = roots(logN)
    e = rot_group(logN)
    k = np.nonzero(m)[0]
    mk = m[k]
    re, im = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    for j0 in range(0, n, block):
        t = (e[j0:j0 + block, None] * k[None, :]) % (2 * N)
        re[j0:j0 + block] = (cs[t] * mk[None, :]).sum(axis=1)
        im[j0:j0 + block] = (sn[t] * mk[None, :]).sum(axis=1)
    return re, im


def _bitrev(n):
    bits = n.bit_length() - 1
    r = np.zeros(n, dtype=np.int64)
    for b in range(bits):
        r |= ((np.arange(n) >> b) & 1) << (bits - 1 - b)
    return r


def fft_slots(m, logN):
    """exact_slots through the radix-2 network (u_k = m_k + i m_(k+n), bit-reversed, stages LEN = 2 .. n with the root zeta^(e_J n / LEN ... ))"""
    N = 1 << logN
    n = N // 2
    m = np.asarray(m).astype(LD)
    cs, sn = roots(logN)
    e = rot_group(logN)
    br = _bitrev(n)
    re, im = m[:n][br].copy(), m[n:][br].copy()
    ln = 2
    while ln <= n:
        h = ln // 2
        t = (e[:h] % (4 * ln)) * (n // ln)
        wr, wi = cs[t], sn[t]
        re2, im2 = re.reshape(-1, ln), im.reshape(-1, ln)
        ar, ai, br_, bi = re2[:, :h].copy(), im2[:, :h].copy(), re2[:, h:], im2[:, h:]
        vr, vi = br_ * wr - bi * wi, br_ * wi + bi * wr
        re2[:, :h], im2[:, :h], re2[:, h:], im2[:, h:] = ar + vr, ai + vi, ar - vr, ai - vi
        ln *= 2
    return re, im


def fft_coeffs(z, logN):
    """exact_coeffs through the inverse network"""
    N = 1 << logN
    n = N // 2
    z = np.asarray(z)
    cs, sn = roots(logN)
    e = rot_group(logN)
    re, im = z.real.astype(LD).copy(), z.imag.astype(LD).copy()
    ln = n
    while ln >= 2:
        h = ln // 2
        t = (e[:h] % (4 * ln)) * (n // ln)
        wr, wi = cs[t], -sn[t]
        re2, im2 = re.reshape(-1, ln), im.reshape(-1, ln)
        ar, ai, br_, bi = re2[:, :h].copy(), im2[:, :h].copy(), re2[:, h:].copy(), im2[:, h:].copy()
        dr, di = ar - br_, ai - bi
        re2[:, :h], im2[:, :h] = ar + br_, ai + bi
        re2[:, h:], im2[:, h:] = dr * wr - di * wi, dr * wi + di * wr
        ln //= 2
    br = _bitrev(n)
    out = np.empty(N, dtype=LD)
    out[:n][br] = re
    out[n:][br] = im
    return out / LD(n)


def round_exact(x):
    """rint of a longdouble array, ties to even, as Python integers (object array)"""
    r = np.rint(np.asarray(x, dtype=LD))
    return np.array([int(v) for v in r], dtype=object)


def encode_int(z, logN, scale, coeffs=exact_coeffs):
    """c_k = rint(Delta m_k): Python integers (object array of length N)"""
    return round_exact(coeffs(z, logN) * LD(scale))


def residues(c, q):
    return np.array([int(v) % q for v in c], dtype=np.uint64)


def encode_limbs(orc, z, scale, mod_ids, coeffs=exact_coeffs):
    """the plaintext of z on the moduli mod_ids of an Oracle: evaluation form, [len(mod_ids)][N]"""
    logN = orc.N.bit_length() - 1
    c = encode_int(z, logN, scale, coeffs)
    a = np.stack([residues(c, orc.moduli[m]) for m in mod_ids])
    return orc.ntt(list(mod_ids), a)


def centre(x, q):
    return np.array([int(v) if int(v) <= (q - 1) // 2 else int(v) - q for v in x], dtype=object)


def decode_int(c, logN, scale, slots=exact_slots):
    """slots (complex128) of integer coefficients c at scale Delta"""
    m = np.array([LD(int(v)) for v in c], dtype=LD) / LD(scale)
    re, im = slots(m, logN)
    return re.astype(np.float64) + 1j * im.astype(np.float64)


def decode_limb(orc, x, mod_id, scale, slots=exact_slots):
    """slots of ONE evaluation-form limb-poly modulo q_(mod_id)"""
    logN = orc.N.bit_length() - 1
    c = orc.ntt([mod_id], np.asarray(x, dtype=np.uint64)[None, :], inverse=True)[0]
    return decode_int(centre(c, orc.moduli[mod_id]), logN, scale, slots)
