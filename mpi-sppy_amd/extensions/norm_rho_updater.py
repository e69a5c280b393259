"""NormRhoUpdater — adaptive rho from the primal / dual residual norms, on the
device (mirrors ``mpisppy/extensions/norm_rho_updater.py:12-165``; same
options, keys and defaults).

The reference's ``miditer`` loops over every local scenario and nonant in
Python; written against the per-scenario views that is one device store per
(scenario, nonant).  Here it is three short launches and one small all-reduce
per PH iteration, with no device-to-host read unless ``verbose``:

  _compute_primal_residual_norm (:55-96)   phx_node_absdev (wt = the scenario
                                           probabilities) + ONE all-reduce of
                                           the [NNS + 1] buffer
  _compute_dual_residual_norm (:98-104),
  the rule (:128-143), _snapshot_avg       phx_norm_rho (rule kernel per (node,
                                           slot) entry, then rho scaled in place)

The next solve picks the new rho up through ``_set_ph_terms``.  W is not
rescaled when rho changes (the reference does not either).

A plain ``NormRhoUpdater`` that is not ``verbose`` does not keep the run on
the host loop: ``PHBase._iterk_native`` hands these buffers to
``phx_iterk_norm_rho``, which runs the same update inside the device loop
 and leaves this object in the state ``miditer`` would have.
A subclass that overrides a loop hook, ``verbose``, a ``MultiExtension`` or
``iterk_solver_options {"native_loop": 0}`` keep the host loop.
"""
import ctypes

import torch

from .. import _native
from .extension import Extension

_norm_rho_defaults = {'convergence_tolerance': 1e-4,
                      'rho_decrease_multiplier': 2.0,
                      'rho_increase_multiplier': 2.0,
                      'primal_dual_difference_factor': 100.,
                      'iterations_converged_before_decrease': 0,
                      'rho_converged_decrease_multiplier': 1.1,
                      'rho_update_stop_iterations': None,
                      'verbose': False,
                      }

_attr_to_option_name_map = {
    '_tol': 'convergence_tolerance',
    '_rho_decrease': 'rho_decrease_multiplier',
    '_rho_increase': 'rho_increase_multiplier',
    '_primal_dual_difference_factor': 'primal_dual_difference_factor',
    '_required_converged_before_decrease': 'iterations_converged_before_decrease',
    '_rho_converged_residual_decrease': 'rho_converged_decrease_multiplier',
    '_stop_iter_rho_update': 'rho_update_stop_iterations',
    '_verbose': 'verbose',
}

ACTIONS = {1: "Increasing", 2: "Decreasing", 3: "Converged, Decreasing"}


class NormRhoUpdater(Extension):

    # set before ph_main: the device loop keeps every iteration's actions in
    # action_log, int32 [PHIterLimit][NNS], row k-1 for iteration k (zeros where
    # an iteration made no update); the host loop keeps no log
    log_actions = False
    action_log = None

    def __init__(self, ph):
        super().__init__(ph)
        self.ph = ph
        self.norm_rho_options = \
            ph.options['norm_rho_options'] if 'norm_rho_options' in ph.options else dict()
        self._set_options()
        self.ph._mpisppy_norm_rho_update_inuse = True  # allow NormRhoConverger
        # device buffers, allocated once: the residuals (+ their total), the
        # actions, the x-bar snapshot and the tile partials of the reduction
        f64 = torch.float64
        nns = max(ph.NNS, 1)
        self._primal = torch.zeros(nns + 1, dtype=f64, device=ph.device)
        self._dual = torch.zeros(nns, dtype=f64, device=ph.device)
        self._action = torch.zeros(nns, dtype=torch.int32, device=ph.device)
        self._prev_avg = torch.zeros(nns, dtype=f64, device=ph.device)
        self._partial = torch.zeros(max(int(ph._tree.npart), 1), dtype=f64, device=ph.device)
        self._have_prev = False
        self._opts = _native.NormRhoOpts()
        self._opts.tol = float(self._tol)
        self._opts.rho_increase = float(self._rho_increase)
        self._opts.rho_decrease = float(self._rho_decrease)
        self._opts.pd_factor = float(self._primal_dual_difference_factor)
        self._opts.conv_decrease = float(self._rho_converged_residual_decrease)

    def _set_options(self):
        options = self.norm_rho_options
        for attr_name, opt_name in _attr_to_option_name_map.items():
            setattr(self, attr_name, options[opt_name] if opt_name in options else _norm_rho_defaults[opt_name])

    def _snapshot_avg(self, ph):
        self._prev_avg.copy_(ph._xbar_node)
        self._have_prev = True

    def _iterk_rho_args(self, max_iterations):
        """phx_iterk_rho over this object's buffers: what the device loop needs to
        run miditer's update itself (PHBase._iterk_native)."""
        ph = self.ph
        r = _native.IterkRho()
        r.opts = self._opts
        r.decrease_from_iter = int(self._required_converged_before_decrease)
        r.stop_after_iter = -1 if self._stop_iter_rho_update is None else int(self._stop_iter_rho_update)
        r.have_prev = int(self._have_prev)
        r.prob, r.partial = ph._prob.data_ptr(), self._partial.data_ptr()
        r.primal, r.xbar_prev = self._primal.data_ptr(), self._prev_avg.data_ptr()
        r.dual_out, r.action_out = self._dual.data_ptr(), self._action.data_ptr()
        r.action_log = None
        if self.log_actions:
            self.action_log = torch.zeros((max(max_iterations, 1), max(ph.NNS, 1)), dtype=torch.int32,
                                          device=ph.device)
            r.action_log = self.action_log.data_ptr()
        return r

    def pre_iter0(self):
        pass

    def post_iter0(self):
        pass

    def miditer(self):
        ph = self.ph
        ph_iter = ph._PHIter
        if self._stop_iter_rho_update is not None and \
                (ph_iter > self._stop_iter_rho_update):
            return
        if ph.NNS == 0 or ph.batch.nonant.N == 0:
            return
        if not self._have_prev:
            self._snapshot_avg(ph)
            return
        ph._settle()          # (x final: a no-op after convergence_diff, where iterk_loop calls this)
        lib = ph._native
        lib.check(ph._ctx, lib.node_absdev(ph._ctx, ctypes.byref(ph._tree), ph._x.data_ptr(),
                                           ph._xbar_node.data_ptr(), ph._prob.data_ptr(), 0,
                                           self._partial.data_ptr(), self._primal.data_ptr(), ph._stream()),
                  "node_absdev")
        ph.mpicomm.allreduce_(self._primal)
        self._opts.allow_decrease = int(ph_iter >= self._required_converged_before_decrease)
        lib.check(ph._ctx, lib.norm_rho(ph._ctx, ctypes.byref(ph._tree), ctypes.byref(self._opts),
                                        self._primal.data_ptr(), ph._xbar_node.data_ptr(),
                                        self._prev_avg.data_ptr(), ph._xbar_idx_t.data_ptr(),
                                        ph._rho.data_ptr(), self._dual.data_ptr(), self._action.data_ptr(),
                                        ph._stream()), "norm_rho")
        ph._bump()
        if self._verbose:
            self._report(ph)

    def _report(self, ph):
        """The reference's table (:144-157) for the first local scenario."""
        primal = self._primal.cpu().numpy()
        dual = self._dual.cpu().numpy()
        action = self._action.cpu().numpy()
        if ph.cylinder_rank != 0 or ph._S == 0:
            return
        rho = ph._host("rho")
        names = ph.batch.nonant.var_names
        first = True
        for j in range(ph.batch.nonant.N):
            e = int(ph._xbar_idx[j, 0])
            if action[e] == 0:
                continue
            if first:
                first = False
                print("Updating rho values:\n%21s %40s %16s %16s %16s"
                      % ("Action", "Variable", "Primal Residual", "Dual Residual", "New Rho"))
            print("%21s %40s %16g %16g %16g" % (ACTIONS[int(action[e])], names[j], primal[e], dual[e], rho[j, 0]))

    def enditer(self):
        pass

    def post_everything(self):
        pass
