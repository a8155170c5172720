"""FakeOps with the per-superchain reduction of nested R-hat (include/bkhip.h: bk_superchain_moments), restated in NumPy
in the DEVICE's summation order -- TEST INFRASTRUCTURE ONLY.

Every sum of a superchain (of mu, of M2 / (n - 1), of (mu - s)^2 about the ROUNDED s: the centred form) takes the order the
kernel's comment states for its M:
  M = 2^j <= 64   the xor butterfly with strides 1, 2, .. M / 2 (butterfly_sum);
  M > 64          thread t adds m = t, t + 256, .. in order, the 256 sums are halved 128, 64, .. 1 (tree256_segment_sum);
  any other M     sequentially in m (sequential_sum).
"""
import numpy as np

from tests.fake_ops import FakeOps

WAVE = 64


def regime(M):
    """'seg' (k_superchain_seg), 'wg' (k_superchain_wg) or 'lane' (k_superchain_lane): the launch bk_superchain_moments picks."""
    if M <= WAVE and M & (M - 1) == 0:
        return "seg"
    return "wg" if M > WAVE else "lane"


def butterfly_sum(x):
    """[.., M] -> [..]: v = v + v[m ^ stride] for stride = 1, 2, .. M / 2 (every lane ends with the same bits)."""
    M = x.shape[-1]
    v = x.copy()
    m = np.arange(M)
    stride = 1
    while stride < M:
        v = v + v[..., m ^ stride]
        stride <<= 1
    return v[..., 0]


def tree256_segment_sum(x):
    """[.., M] -> [..]: thread t adds elements t, t + 256, .. in order (0.0 first), then the LDS tree 128, 64, .. 1."""
    M = x.shape[-1]
    rounds = -(-M // 256)
    pad = np.zeros(x.shape[:-1] + (rounds * 256,))
    pad[..., :M] = x
    red = np.zeros(x.shape[:-1] + (256,))
    for r in range(rounds):
        red = red + pad[..., r * 256:(r + 1) * 256]
    w = 128
    while w > 0:
        red[..., :w] = red[..., :w] + red[..., w:2 * w]
        w >>= 1
    return red[..., 0]


def sequential_sum(x):
    s = np.zeros(x.shape[:-1])
    for m in range(x.shape[-1]):
        s = s + x[..., m]
    return s


SUMS = {"seg": butterfly_sum, "wg": tree256_segment_sum, "lane": sequential_sum}


def superchain_moments_ref(mean, m2, n, M, total=None):
    """bk_superchain_moments on NumPy [D, C] arrays -> (s, w), [D, C // M] each.  total: the sum over a superchain's M values."""
    D, C = mean.shape
    assert M >= 1 and n >= 1 and C % M == 0
    total = SUMS[regime(M)] if total is None else total
    x = np.ascontiguousarray(mean).reshape(D, C // M, M)
    s = total(x) / float(M)
    dv = x - s[..., None]
    bt = total(dv * dv) / (float(M) - 1.0) if M > 1 else np.zeros_like(s)
    if n > 1:
        wt = total(np.ascontiguousarray(m2).reshape(D, C // M, M) / float(n - 1)) / float(M)
    else:
        wt = np.zeros_like(s)
    return s, bt + wt


class NestedFakeOps(FakeOps):
    name = "fake-cpu-nested"

    def superchain_moments(self, mean, m2, n, M, s_out, w_out):
        self._count("superchain_moments")
        D, C = mean.shape
        if M < 1 or n < 1 or C % M != 0 or (m2 is None and n > 1):
            raise ValueError("bk_superchain_moments: BK_E_ARG")
        assert tuple(s_out.shape) == tuple(w_out.shape) == (D, C // M)
        if C == 0 or D == 0:
            return
        s, w = superchain_moments_ref(mean.numpy(), None if n == 1 else m2.numpy(), n, M)
        s_out.numpy()[...] = s
        w_out.numpy()[...] = w
