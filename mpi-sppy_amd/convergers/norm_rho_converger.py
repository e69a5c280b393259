"""NormRhoConverger — stop when log(sum_s p_s sum_j rho[j][s]) drops below
``convthresh`` (mirrors ``mpisppy/convergers/norm_rho_converger.py:12-56``).

``_compute_rho_norm`` (:23-29) is one reduction on the device (phx_rho_sums)
and one all-reduce; the scalar is read back once per PH iteration.
"""
import math

import torch

from .converger import Converger


class NormRhoConverger(Converger):

    def __init__(self, ph):
        super().__init__(ph)
        if 'norm_rho_converger_options' in ph.options and \
                'verbose' in ph.options['norm_rho_converger_options'] and \
                ph.options['norm_rho_converger_options']['verbose']:
            self._verbose = True
        else:
            self._verbose = False
        self.ph = ph
        self._sums = torch.zeros(2, dtype=torch.float64, device=ph.device)

    def _compute_rho_norm(self, ph):
        lib = ph._native
        ph._settle()
        lib.check(ph._ctx, lib.rho_sums(ph._ctx, ph._rho.data_ptr(), ph._prob.data_ptr(), None, None, None,
                                        self._sums.data_ptr(), ph._stream()), "rho_sums")
        if ph.n_proc > 1:
            ph.mpicomm.allreduce_(self._sums)
            return float(self._sums.cpu().numpy()[0])
        return float(ph._read_small(self._sums)[0])

    def is_converged(self):
        """ check for convergence
        Returns:
           converged?: True if converged, False otherwise
        """
        # This will never do anything unless the norm rho updater is also used
        if not hasattr(self.ph, "_mpisppy_norm_rho_update_inuse") \
                or not self.ph._mpisppy_norm_rho_update_inuse:
            raise RuntimeError("NormRhoConverger can only be used if NormRhoUpdater is")

        log_rho_norm = math.log(self._compute_rho_norm(self.ph))

        ret_val = log_rho_norm < self.ph.options['convthresh']
        self.conv = log_rho_norm
        if self._verbose and self.ph.cylinder_rank == 0:
            print(f"log(|rho|) = {log_rho_norm}")
            if ret_val:
                print("Norm rho convergence check passed")
            else:
                print("Adaptive rho convergence check failed "
                      f"(requires log(|rho|) < {self.ph.options['convthresh']}")
                print("Continuing PH with updated rho")
        return ret_val
