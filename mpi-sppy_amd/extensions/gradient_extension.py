"""Gradient_extension — PH with gradient-based, cost-proportional rho, on the
device (mirrors ``mpisppy/extensions/gradient_extension.py:18-109``; same
option, ``options["gradient_extension_options"]["cfg"]``, and hook logic).

The reference's ``miditer`` writes the gradient cost and the rho to CSV files in
the working directory, reads them back through ``Set_Rho.rho_setter`` and
installs rho with one write per (scenario, nonant).  Here nothing leaves the
device but the two scalars the trigger compares:

  WTracker.W_diff (utils/wtracker.py:134-157)    phx_w_absdiff + ONE all-reduce
                                                 of a scalar
  Find_Grad.write_grad_cost at _PHIter == 1      a [N][S] device tensor, built once
  write_grad_rho + rho_setter + rho writes       Find_Rho.compute_rho_device:
                                                 phx_cost_rho_stats, two
                                                 all-reduces, phx_cost_rho_apply

The rule uses the reference's default, scenario-dependent denominator.  rho is
recomputed when the W difference stalls, |last - curr| / last <= 0.05; a last
value of 0 means no update (numpy's inf / nan compares False in the reference).
An entry whose rho would not be finite keeps its rho (see utils/find_rho.py).
No temporary files are written.  ``_display_rho_values`` prints as the
reference's, when the run is verbose (it reads rho back).

A per-iteration hook: runs with it use the host loop (NormRhoUpdater's update
is the one that runs inside the device loop).
"""
import types

import torch

from ..spbase import _global_toc
from ..utils import find_rho, gradient
from ..utils.find_rho import cfg_get
from .extension import Extension


class Gradient_extension(Extension):
    """
    Args:
       opt (PHBase object): gives the problem

    Attributes:
       grad_object (Find_Grad object): gradient object
    """

    def __init__(self, opt, comm=None):
        super().__init__(opt)
        if opt._bundles is not None:
            raise NotImplementedError("Gradient_extension with bundles_per_rank is not supported")
        self.cylinder_rank = self.opt.cylinder_rank
        self.cfg = opt.options["gradient_extension_options"]["cfg"]
        self.grad_object = gradient.Find_Grad(opt, self.cfg)
        # (the rule's parameters only: the device path reads no cost file)
        self.rho_object = find_rho.Find_Rho(opt, types.SimpleNamespace(
            order_stat=cfg_get(self.cfg, "order_stat"),
            rho_relative_bound=cfg_get(self.cfg, "rho_relative_bound")))
        self.primal_conv_cache = []
        self.dual_conv_cache = []
        self._cost_t = None
        self._W_prev = None
        self._wdiff = torch.zeros(1, dtype=torch.float64, device=opt.device)

    def _display_rho_values(self):
        ph = self.opt
        if ph._S == 0 or ph.batch.nonant.N == 0:
            return
        rho_list = ph._rho.view(-1, ph._S)[:, 0].cpu().tolist()
        print(ph.local_scenario_names[0], 'rho values: ', rho_list)

    def W_diff(self):
        """mean |W - W_prev| over the local (scenario, nonant) entries, summed over
        ranks and divided by their number (WTracker.W_diff).  The first call
        snapshots W and returns 0."""
        ph = self.opt
        ph._settle()
        if self._W_prev is None:
            self._W_prev = ph._W.clone()
            return 0.0
        count = ph.batch.nonant.N * ph._S
        if count > 0:
            lib = ph._native
            lib.check(ph._ctx, lib.w_absdiff(ph._ctx, ph._W.data_ptr(), self._W_prev.data_ptr(),
                                             self._wdiff.data_ptr(), ph._stream()), "w_absdiff")
            self._wdiff.div_(float(count))
        else:
            self._wdiff.zero_()
        ph.mpicomm.allreduce_(self._wdiff)
        return float(ph._read_small(self._wdiff)[0]) / ph.n_proc

    def _update_rho_dual_based(self):
        curr_conv, last_conv = self.dual_conv_cache[-1], self.dual_conv_cache[-2]
        if last_conv == 0:
            return False
        dual_diff = abs((last_conv - curr_conv) / last_conv)
        return (dual_diff <= 0.05)

    def _update_rho(self):
        """rho of every (node, slot) entry from the gradient cost, installed on the device."""
        return self.rho_object.compute_rho_device(self._cost_t, indep_denom=False)

    def pre_iter0(self):
        pass

    def post_iter0(self):
        _global_toc("Using gradient-based rho setter", self.cylinder_rank == 0 and self.opt.options["verbose"])
        self.primal_conv_cache.append(self.opt.convergence_diff())
        self.dual_conv_cache.append(self.W_diff())
        if self.opt.options["verbose"] and self.cylinder_rank == 0:
            self._display_rho_values()

    def miditer(self):
        self.primal_conv_cache.append(self.opt.convergence_diff())
        self.dual_conv_cache.append(self.W_diff())
        if self.opt._PHIter == 1:
            self._cost_t = self.grad_object.grad_cost_device()
        if self.opt._PHIter >= 0 and (self._update_rho_dual_based()):
            if self._cost_t is None:
                self._cost_t = self.grad_object.grad_cost_device()
            self._update_rho()
            if self.opt.options["verbose"] and self.cylinder_rank == 0:
                self._display_rho_values()

    def enditer(self):
        pass

    def post_everything(self):
        pass
