"""PrimalDualConverger — the primal / dual residual stop test (mirrors
``mpisppy/convergers/primal_dual_converger.py:9-137``):

    primal gap = sum_s sum_j prob_coeff(j,s) |x(j,s) - xbar|      (:58-85)
    dual gap   = sum_s sum_j rho(j,s) |xbar_t - xbar_{t-1}|       (:87-110)
    converged when max(primal gap, dual gap) <= tol

Both are reductions on the device (phx_node_absdev's total with the
prob_coeff weights, phx_rho_sums), all-reduced together and read back once per
PH iteration.  ``tracking`` (pandas / matplotlib output of the reference) is
not supported.
"""
import ctypes

import torch

from .converger import Converger


class PrimalDualConverger(Converger):
    """ Convergence checker for the primal-dual metrics.
        Primal convergence is measured as weighted sum over all scenarios s
        p_{s} * ||x_{s} - \\bar{x}||_1.
        Dual convergence is measured as
        rho * ||\\bar{x}_{t} - \\bar{x}_{t-1}||_1
    """
    def __init__(self, ph):
        super().__init__(ph)
        self.options = ph.options.get('primal_dual_converger_options', {})
        self._verbose = self.options.get('verbose', False)
        self._ph = ph
        self.convergence_threshold = self.options.get('tol', 1)
        self.tracking = self.options.get('tracking', False)
        if self.tracking:
            raise NotImplementedError("primal_dual_converger_options['tracking'] is not supported")
        self._rank = self._ph.cylinder_rank
        # device buffers, allocated once: the previous x-bar, the per-entry
        # residuals (+ total), the tile partials, the two gaps
        f64 = torch.float64
        nns = max(ph.NNS, 1)
        self.prev_xbars = torch.zeros(nns, dtype=f64, device=ph.device)
        self._get_xbars()
        self._primal = torch.zeros(nns + 1, dtype=f64, device=ph.device)
        self._partial = torch.zeros(max(int(ph._tree.npart), 1), dtype=f64, device=ph.device)
        self._sums = torch.zeros(2, dtype=f64, device=ph.device)
        self._gaps = torch.zeros(2, dtype=f64, device=ph.device)
        self.primal_gap = self.dual_gap = None

    def _get_xbars(self):
        """Snapshot the current x-bar buffer (device copy)."""
        self.prev_xbars.copy_(self._ph._xbar_node)

    def _compute_gaps(self):
        """(primal gap, dual gap), all-reduced."""
        ph = self._ph
        lib = ph._native
        ph._settle()
        lib.check(ph._ctx, lib.node_absdev(ph._ctx, ctypes.byref(ph._tree), ph._x.data_ptr(),
                                           ph._xbar_node.data_ptr(), ph._pc.data_ptr(), 1,
                                           self._partial.data_ptr(), self._primal.data_ptr(), ph._stream()),
                  "node_absdev")
        lib.check(ph._ctx, lib.rho_sums(ph._ctx, ph._rho.data_ptr(), ph._prob.data_ptr(), ph._xbar_node.data_ptr(),
                                        self.prev_xbars.data_ptr(), ph._xbar_idx_t.data_ptr(),
                                        self._sums.data_ptr(), ph._stream()), "rho_sums")
        self._gaps[0].copy_(self._primal[ph.NNS])
        self._gaps[1].copy_(self._sums[1])
        if ph.n_proc > 1:
            ph.mpicomm.allreduce_(self._gaps)
            v = self._gaps.cpu().numpy()
        else:
            v = ph._read_small(self._gaps)
        return float(v[0]), float(v[1])

    def is_converged(self):
        """ check for convergence
        Returns:
           converged?: True if converged, False otherwise
        """
        ph = self._ph
        if ph.NNS == 0 or ph.batch.nonant.N == 0:
            primal_gap = dual_gap = 0.0
        else:
            primal_gap, dual_gap = self._compute_gaps()
        self._get_xbars()
        self.primal_gap, self.dual_gap = primal_gap, dual_gap
        ret_val = max(primal_gap, dual_gap) <= self.convergence_threshold

        if self._verbose and self._rank == 0:
            print(f"primal gap = {round(primal_gap, 5)}, dual gap = {round(dual_gap, 5)}")

            if ret_val:
                print("Dual convergence check passed")
            else:
                print("Dual convergence check failed "
                      f"(requires primal + dual gaps) <= {self.convergence_threshold}")
        return ret_val
