"""AdaptFakeOps with the entry points of the dense-metric adaptation (include/bkhip.h: bk_cov_accumulate,
bk_cov_accumulate_work_elems, bk_cov_k_chunk) in NumPy -- TEST INFRASTRUCTURE ONLY.

Plain Xc @ Xc.T in float64, symmetrised by construction; the summation order of the MFMA tiles and slabs is NOT restated, so
comparisons between the library and this stand-in are by tolerance, like the dense-metric sampler tests."""
import numpy as np
import torch

from tests.fake_ops_adapt import AdaptFakeOps


class DenseAdaptFakeOps(AdaptFakeOps):
    name = "fake-cpu-dense-adapt"

    @staticmethod
    def cov_k_chunk(D):
        return 128

    def cov_work(self, D, C):
        return torch.empty(1, dtype=torch.float64)

    def cov_accumulate(self, X, center, S, s, work):
        self._count("cov_accumulate")
        x = X.numpy()
        xc = x if center is None else x - center.numpy()[:, None]
        g = xc @ xc.T
        low = np.tril(S.numpy()) + np.tril(g)   # the lower triangle is what is read; both are written from it
        S.numpy()[...] = low + np.tril(low, -1).T
        s.numpy()[...] = s.numpy() + xc.sum(axis=1)
