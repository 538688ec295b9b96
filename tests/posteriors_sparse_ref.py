"""The semantics of the sparse posteriors (include/tdnnf_hip.h, "sparse posteriors") in numpy, taken literally: per frame the candidates are
the columns with value > min_post (strict: a zero, a negative value and a NaN never are), kept are all of them if there are at most K and
otherwise the first K under a stable sort on (-value, pdf); the kept pairs are written in ascending pdf order, the other slots hold (-1, 0).
tests/test_posteriors_sparse_cpu.py pins it on hand-written rows; tests/test_gpu_posteriors_sparse.py holds the library to it, bit for bit."""
import numpy as np


def sparsify(block, pdfs, min_post, K):
    """block [T, D] float32 (a compact posterior block), pdfs [D] ascending -> (pdf [T, K] int32, post [T, K] float32, count [T] int32,
    n [T] int32: the candidates of each frame, of which count = min(n, K) are kept)"""
    block = np.asarray(block, np.float32)
    pdfs = np.asarray(pdfs, np.int32).reshape(-1)
    T, D = block.shape
    assert len(pdfs) == D and (np.diff(pdfs) > 0).all() and K >= 1 and np.isfinite(min_post) and min_post >= 0
    pdf = np.full((T, K), -1, np.int32)
    post = np.zeros((T, K), np.float32)
    count, n = np.zeros(T, np.int32), np.zeros(T, np.int32)
    for t in range(T):
        cand = np.nonzero(block[t] > np.float32(min_post))[0]  # ascending columns = ascending pdfs
        n[t] = len(cand)
        if len(cand) > K:
            order = np.argsort(-block[t, cand], kind="stable")  # among equal values the lower pdf stays first
            cand = np.sort(cand[order[:K]])
        count[t] = len(cand)
        pdf[t, :len(cand)] = pdfs[cand]
        post[t, :len(cand)] = block[t, cand]
    return pdf, post, count, n
