"""User-defined residual blocks on poses beside the typed device tables (``Options.hybrid_blocks``).

A block without a typed ``KIND`` whose parameters are all poses of the problem's group (at most ``MAX_BLOCK_POSES`` of
them) is evaluated here, through its own ``evaluate(params, compute_jacobians)``, while every typed block stays in the
device tables.  What the device receives from such a block is its share of the normal equations, cut into pose-pair
rows of the layout the pose-factor kernels stage per edge (csrc/ps_k_linearize.h: k_factor_pass), so that
``k_factor_assemble`` adds them into S and g with the edges and priors:

    [H11 | H12 | H22 | g1 | g2]      (3 D^2 + 2 D doubles, D x D blocks row-major, g = -J~^T e~)

A block on the distinct variable poses (a, b, c, ...) becomes the rows (a, b), (a, c), ..., (b, c), ...; one variable
pose gives the single row (-1, a), the prior convention of k_factor_pass.  Every diagonal block H_aa and gradient piece
is carried by exactly one row (the first that holds the pose), the other rows carry zeros there: the rows add up to the
block's J~^T J~ and -J~^T e~.  Constant poses contribute no rows.
"""
import numpy as np

MAX_BLOCK_POSES = 8


def block_rows(var):
    """Pose-pair rows [(i, j)] of a block on the distinct variable poses `var` (in block order)."""
    if len(var) == 1:
        return [(-1, var[0])]
    return [(var[a], var[b]) for a in range(len(var)) for b in range(a + 1, len(var))]


def row_width(dof):
    return 3 * dof * dof + 2 * dof


class HostBlocks:
    """The user blocks of a hybrid LoweredProblem, evaluated at pose rows (pyslam_amd/lowering.py packing).

    `blocks`, `keys`, `losses`: the Problem's registries (read at every evaluation: a block swapped for another on the same
    poses takes effect as the reference's walk would have it); `param_dict`: gives the pose classes the blocks receive."""

    def __init__(self, lp, blocks, keys, losses, param_dict):
        self.lp = lp
        self.blocks, self.keys, self.losses = blocks, keys, losses
        self.dof = lp.dof
        n = 3 if lp.dof == 6 else 2
        self._n = n
        sample = param_dict[lp.pose_keys[int(lp.h_pose[0])]] if lp.h_pose.size else None
        self._pose_cls = type(sample) if sample is not None else None
        self._rot_cls = type(sample.rot) if sample is not None else None
        rid = lp.pose_rid
        self._items = []            # per block: (block index, pose index per key, variable flag per key, distinct variable poses)
        for b, blk in enumerate(lp.h_blocks):
            pix = [int(p) for p in lp.h_pose[lp.h_pose_ptr[b]:lp.h_pose_ptr[b + 1]]]
            want = [bool(rid[p] >= 0) for p in pix]
            var = []
            for p, w in zip(pix, want):
                if w and p not in var:
                    var.append(p)
            self._items.append((int(blk), pix, want, var))
        self.num_rows = int(lp.h_i.size)

    def _poses(self, rows, needed):
        n, out = self._n, {}
        for p in needed:
            r = rows[p]
            out[p] = self._pose_cls(self._rot_cls(np.array(r[:n * n]).reshape(n, n)), np.array(r[n * n:n * n + n]))
        return out

    def _params(self, rows):
        needed = sorted({p for _, pix, _, _ in self._items for p in pix})
        return self._poses(rows, needed)

    def evaluate(self, poses):
        """Rows (num_rows, 3 D^2 + 2 D) of the linearisation at `poses`, and the cost of the blocks with a variable pose
        (reference problem.py:338-360: ``_host_jacobian``'s sum).  Same arithmetic per block as ``Problem._host_jacobian``:
        s = sqrt(loss.weight(r)), J~ = s J, e~ = s r; a pose listed twice adds its Jacobians up."""
        D, DD = self.dof, self.dof * self.dof
        rows = np.zeros((self.num_rows, row_width(D)))
        objs = self._params(poses)
        cost, k = 0., 0
        for blk, pix, want, var in self._items:
            if not var:
                continue
            block, loss = self.blocks[blk], self.losses[blk]
            residual, jacobians = block.evaluate([objs[p] for p in pix], want)
            residual = np.atleast_1d(residual).reshape(-1)
            s = np.sqrt(np.asarray(loss.weight(residual), dtype=float)).reshape(-1)
            nres = residual.size
            A = {p: np.zeros((nres, D)) for p in var}
            for p, w, jac in zip(pix, want, jacobians):
                if w and jac is not None:
                    A[p] = A[p] + s[:, None] * np.asarray(jac, dtype=float).reshape(nres, -1)
            e = s * residual
            cost += np.sum(loss.loss(residual))
            if len(var) == 1:
                a = A[var[0]]
                rows[k, 2 * DD:3 * DD] = (a.T @ a).ravel()
                rows[k, 3 * DD + D:] = -(a.T @ e)
                k += 1
                continue
            for ia in range(len(var)):
                for ib in range(ia + 1, len(var)):
                    a, b = A[var[ia]], A[var[ib]]
                    rows[k, DD:2 * DD] = (a.T @ b).ravel()
                    if ia == 0:                   # the first row holding pose var[ib] carries its diagonal block
                        rows[k, 2 * DD:3 * DD] = (b.T @ b).ravel()
                        rows[k, 3 * DD + D:] = -(b.T @ e)
                        if ib == 1:               # ... and the very first row that of var[0]
                            rows[k, :DD] = (a.T @ a).ravel()
                            rows[k, 3 * DD:3 * DD + D] = -(a.T @ e)
                    k += 1
        assert k == self.num_rows
        return rows, cost

    def cost(self, poses, include_all_constant=True):
        """Sum of loss.loss(r) over the user blocks at `poses` (blocks whose poses are all constant only with
        `include_all_constant`, as ps_eval_cost)."""
        objs = self._params(poses)
        cost = 0.
        for blk, pix, want, var in self._items:
            if not var and not include_all_constant:
                continue
            residual = self.blocks[blk].evaluate([objs[p] for p in pix])
            cost += np.sum(self.losses[blk].loss(residual))
        return cost
