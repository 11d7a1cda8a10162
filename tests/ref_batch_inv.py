"""NumPy restatement of steps (a) and (b) of the mid-order batched NLL gradient (sgpr_fit_batch_grad_mid, batch.hip), tile by
tile with the kernels' index formulas: L in an npad x npad image (npad = n rounded up to 128, identity padding), U = L^-T in
a second image with U[i, k] = (L^-1)[k, i], the block-doubling recursion over 128-tiles with the ragged last block, the
products T = U11 L21^T parked in the L image's upper triangle, the clipped k ranges, and Ky^-1 = U U^T in lower tiles over L."""
import numpy as np

LEAF = 128


def padded_image(A):
    """A (n x n, SPD) -> (Ky image npad x npad with an identity block as padding, npad, W)"""
    n = A.shape[0]
    npad = (n + LEAF - 1) // LEAF * LEAF
    img = np.eye(npad)
    img[:n, :n] = A
    return img, npad, npad // LEAF


def factor_image(img):
    """what the factorisation leaves: L (lower; zeros above the diagonal) and the inverses of its diagonal 128-blocks"""
    L = np.linalg.cholesky(img)
    W = L.shape[0] // LEAF
    inv = [np.linalg.inv(L[t * LEAF:(t + 1) * LEAF, t * LEAF:(t + 1) * LEAF]) for t in range(W)]
    return L, inv


def tile(M, i, j):
    return M[i * LEAF:(i + 1) * LEAF, j * LEAF:(j + 1) * LEAF]


def u_image(Limg, inv, W):
    """step (a).  Limg is written to (the T blocks, above the diagonal), as on the device.  -> (U image, launches)"""
    npad = W * LEAF
    U = np.zeros((npad, npad))
    for t in range(W):                                   # mid_udiag_kernel: U[i, k] = X[k, i] for k >= i, else 0
        tile(U, t, t)[:] = np.triu(inv[t].T)
    launches = 1
    S = 1
    while S < W:
        npairs = (W - S + 2 * S - 1) // (2 * S)
        for step in (0, 1):
            for bx in range(npairs * S * S):             # mid_inv_level_kernel<step>: blockIdx.x -> (pair, ti, tj)
                p, rem = divmod(bx, S * S)
                ti, tj = rem % S, rem // S
                t1 = 2 * S * p
                t2 = t1 + S
                if t2 + tj >= W:
                    continue                             # past the ragged last block
                ri, cj = t1 + ti, t2 + tj
                if step == 0:                            # T(ti, tj) = sum_{k >= ti} U11[ti, k] L21[tj, k]^T
                    acc = np.zeros((LEAF, LEAF))
                    for k in range(ti, S):
                        acc += tile(U, ri, t1 + k) @ tile(Limg, cj, t1 + k).T
                    tile(Limg, ri, cj)[:] = acc
                else:                                    # U12(ti, tj) = -sum_{k <= tj} T[ti, k] U22[k, tj]
                    acc = np.zeros((LEAF, LEAF))
                    for k in range(tj + 1):
                        acc += tile(Limg, ri, t2 + k) @ tile(U, t2 + k, cj)
                    tile(U, ri, cj)[:] = -acc
            launches += 1
        S *= 2
    return U, launches


def kinv_lower(U, Limg, W):
    """step (b): tile (I, J), I >= J, of Ky^-1 = U U^T summed over k-blocks >= I, written over Limg's lower tiles"""
    t = 0
    for bx in range(W * (W + 1) // 2):                   # mid_kinv_kernel: lower tiles row by row
        t, r = bx, 0
        while t > r:
            t -= r + 1
            r += 1
        acc = np.zeros((LEAF, LEAF))
        for k in range(r, W):
            acc += tile(U, r, k) @ tile(U, t, k).T
        tile(Limg, r, t)[:] = acc
    return Limg
