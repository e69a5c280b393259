"""Gradient cost and gradient-based rho -- mirrors ``mpisppy/utils/gradient.py``
(``Find_Grad`` :44-175): same methods and CSV formats.

The engine's objectives are linear, so the gradient of a scenario's objective
with respect to a nonant is that variable's own objective coefficient, whatever
x is.  The gradient cost is therefore minus the coefficient, in the sense the
scenario creator stated (``batch.c`` / ``batch.sense``), and

* ``xhatpath`` is not needed: the reference fixes the nonants at an xhat and
  solves before it evaluates the gradient (:93-105); for a linear objective the
  result does not depend on the point, so that solve is skipped;
* the reference indexes PyomoNLP's gradient vector by the nonant's *position*
  in the node's list (``grad[ndn_i[1]]``, :79-80), not by the variable's own
  index in the NLP.  Its farmer fixture therefore lists 150 (WHEAT's planting
  cost) for CORN, whose coefficient is 230.  This port uses the variable's own
  coefficient: farmer gives -230, -260, -150 for CORN0, SUGAR_BEETS0, WHEAT0.
"""
import csv
import os

import numpy as np
import torch

from . import find_rho
from .find_rho import cfg_get


class Find_Grad():
    """Interface to compute and write gradient cost

    Args:
       ph_object (PHBase): ph object
       cfg: config object (see find_rho.rho_cfg)

    Attributes:
       c (dict): gradient cost {(scenario name, variable name): value}
    """

    def __init__(self, ph_object, cfg):
        self.ph_object = ph_object
        self.cfg = cfg
        self.c = dict()

    def _slot_costs(self):
        """(N, S) minus the nonants' objective coefficients, as the creator stated them."""
        b = self.ph_object.batch
        cols = b.nonant.slot_col
        c = np.asarray(b.c, dtype=np.float64)
        g = c[:, cols].T if c.ndim == 2 else np.broadcast_to(c[cols][:, None], (len(cols), b.S))
        return -np.ascontiguousarray(g)

    def grad_cost_device(self):
        """The gradient cost as a [N][S] device tensor (what Gradient_extension
        hands to Find_Rho.compute_rho_device; no file, no per-scenario loop)."""
        return torch.as_tensor(self._slot_costs()).to(self.ph_object.device)

    def compute_grad(self, sname, scenario):
        """Gradient cost for a given scenario (a local scenario view).

        Returns:
           grad_cost (dict): {nonant index (ndn, i): gradient cost}
        """
        g = self._slot_costs()
        return {ndn_i: float(g[j, scenario._s]) for j, ndn_i in enumerate(scenario._keys())}

    def find_grad_cost(self):
        """Gradient cost for all scenarios, gathered on cylinder rank 0."""
        if cfg_get(self.cfg, "grad_cost_file") == '':
            pass
        else:
            ph = self.ph_object
            names = ph.batch.nonant.var_names
            local_costs = {}
            for sname, scenario in ph.local_scenarios.items():
                grad_cost = self.compute_grad(sname, scenario)
                for j, ndn_i in enumerate(scenario._keys()):
                    local_costs[(sname, names[j])] = grad_cost[ndn_i]
            costs = ph.mpicomm.gather(local_costs, root=0)
            if ph.cylinder_rank == 0:
                self.c = {key: val for cost in costs for key, val in cost.items()}
            ph.mpicomm.Barrier()

    def write_grad_cost(self):
        """Writes gradient cost for all scenarios."""
        self.find_grad_cost()
        ph = self.ph_object
        if ph.cylinder_rank == 0:
            with open(cfg_get(self.cfg, "grad_cost_file"), 'a') as f:
                writer = csv.writer(f)
                writer.writerow(['#grad cost values'])
                for (key, val) in self.c.items():
                    sname, vname = key[0], key[1]
                    writer.writerow([sname, vname, str(val)])
        ph.mpicomm.Barrier()

    def find_grad_rho(self):
        """rho for all variables from the gradient cost file."""
        grad_cost_file = cfg_get(self.cfg, "grad_cost_file")
        assert grad_cost_file != '', "to compute rho you have to give the name of a csv file (using --grad-cost-file) where grad cost will be written"
        if (not os.path.exists(grad_cost_file)):
            raise RuntimeError('Could not find file {fn}'.format(fn=grad_cost_file))
        self.cfg.whatpath = grad_cost_file
        return find_rho.Find_Rho(self.ph_object, self.cfg).compute_rho()

    def write_grad_rho(self):
        """Writes gradient rho for all variables."""
        grad_rho_file = cfg_get(self.cfg, "grad_rho_file")
        if grad_rho_file == '':
            pass
        else:
            rho_data = self.find_grad_rho()
            if self.ph_object.cylinder_rank == 0:
                with open(grad_rho_file, 'a', newline='') as file:
                    writer = csv.writer(file)
                    writer.writerow(['#grad rho values'])
                    for (vname, rho) in rho_data.items():
                        writer.writerow([vname, rho_data[vname]])
