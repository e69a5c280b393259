"""Cost-proportional rho (the Watson-Woodruff rule) -- mirrors
``mpisppy/utils/find_rho.py`` (``Find_Rho`` :45-218, ``Set_Rho`` :221-259):
same methods, file conventions and messages.

The reference forms ``|cost| / denominator`` per scenario in Python, gathers the
per-scenario lists on rank 0 and takes an order statistic per variable.  Here
the candidates never leave the device: ``compute_rho_device`` is

  phx_cost_rho_stats     sum / count / max / -min of the candidates per (node,
                         slot) entry (the scenario-dependent denominator, or the
                         scenario-independent one from phx_node_absdev)
  two all-reduces        SUM of [sum | count], MAX of [max | -min]
  phx_cost_rho_apply     the order statistic per entry and rho[j][s] = rho_e

with no host read, for any tree.  The dict / file API (``compute_rho``,
``write_rho``) sits on top of it, keeps the reference's two-stage assertion and
reads the per-entry result back once.

Two departures from the reference, both deliberate: an entry whose rho would be
inf or nan (every candidate's denominator zero, or no scenario at all) keeps its
current rho (``kept`` marks it) where the reference would install the inf / nan;
and the cost values parsed from a file are ``float(field.strip())`` (the
reference drops the last two characters of the line, which loses a digit when
the line ends in a bare newline).

``cfg`` is any object with attributes; a missing attribute takes the
reference's default (``rho_cfg`` builds such an object).
"""
import csv
import ctypes
import os
import types

import numpy as np
import torch

from .. import _native

_CFG_DEFAULTS = {"whatpath": "", "rho_file": "", "rho_path": "", "grad_cost_file": "", "grad_rho_file": "",
                 "xhatpath": "", "order_stat": -1.0, "rho_relative_bound": 1e3, "rho_setter": False}


def rho_cfg(**kw):
    """A cfg object for Find_Rho / Find_Grad / Gradient_extension: the reference's
    rho_args / gradient_args attributes with their defaults, overridden by kw."""
    d = dict(_CFG_DEFAULTS)
    d.update(kw)
    return types.SimpleNamespace(**d)


def cfg_get(cfg, name):
    return getattr(cfg, name, _CFG_DEFAULTS[name])


def _node_name(node):
    return node if isinstance(node, str) else node.name


class Find_Rho():
    """Interface to compute rhos from Ws for a given ph object and write them in a file

    Args:
       ph_object (PHBase): ph object
       cfg: config object (see rho_cfg)

    Attributes:
       c (dict): {(scenario name, variable name): cost}, the cost vector of the rule
    """

    def __init__(self, ph_object, cfg):
        self.ph_object = ph_object
        self.cfg = cfg
        self.c = dict()
        self._buf = None
        self.kept = None

        if cfg_get(cfg, "rho_file") == '' and cfg_get(cfg, "grad_rho_file") == '':
            pass
        else:
            whatpath = cfg_get(cfg, "whatpath")
            assert whatpath != '', "to compute rhos you have to give the name of a What csv file (using --whatpath)"
            if (not os.path.exists(whatpath)):
                raise RuntimeError('Could not find file {fn}'.format(fn=whatpath))
            with open(whatpath, 'r') as f:
                for line in f:
                    if (line.startswith('#')):
                        continue
                    line = line.split(',')
                    self.c[(line[0], line[1])] = float(line[2].strip())

    # ------------------------------------------------------------ host views (two-stage)
    def _deviation(self, s, node):
        assert _node_name(node) == "ROOT", "compute rho only works for two stage for now"
        ph = self.ph_object
        x = ph._host("x")[ph.batch.nonant.slot_col, s._s]
        xbar = ph._host("xbar")[ph._xbar_idx[:, s._s]]
        stage1 = ph.batch.nonant.slot_stage == 1
        return (x - xbar)[stage1]

    def _w_denom(self, s, node):
        """The denominator for w-based rho, |x - xbar| (scenario dependent)."""
        return np.abs(self._deviation(s, node))

    def _prox_denom(self, s, node):
        """The denominator corresponding to the proximal term, 2 (x - xbar)^2."""
        return 2 * np.square(self._deviation(s, node))

    def _grad_denom_device(self):
        """[NNS] max(1/rho_relative_bound, sum_s prob_coeff |x - xbar|), all-reduced, on the device."""
        ph = self.ph_object
        b = self._buffers()
        ph._settle()
        ph.Compute_Xbar()
        lib = ph._native
        lib.check(ph._ctx, lib.node_absdev(ph._ctx, ctypes.byref(ph._tree), ph._x.data_ptr(),
                                           ph._xbar_node.data_ptr(), ph._pc.data_ptr(), 1,
                                           b["partial"].data_ptr(), b["denom"].data_ptr(), ph._stream()),
                  "node_absdev")
        ph.mpicomm.allreduce_(b["denom"])
        b["denom"].clamp_(min=1.0 / float(cfg_get(self.cfg, "rho_relative_bound")))
        return b["denom"]

    def _grad_denom(self):
        """The scenario independent denominator in the WW heuristic (rank 0; None elsewhere)."""
        ph = self.ph_object
        assert not ph.multistage, "compute rho only works for two stage for now"
        d = self._grad_denom_device()
        if ph.cylinder_rank == 0:
            return d[:ph.NNS].cpu().numpy()

    def _order_stat(self, rho_list):
        """A scenario independent rho from a list of rhos."""
        alpha = cfg_get(self.cfg, "order_stat")
        assert alpha != -1.0, "you need to set the order statistic parameter for rho using --order-stat"
        assert (alpha >= 0 and alpha <= 1), "0 is the min, 0.5 the average, 1 the max"
        rho_mean, rho_min, rho_max = np.mean(rho_list), np.min(rho_list), np.max(rho_list)
        if alpha == 0.5:
            return rho_mean
        if alpha < 0.5:
            return (rho_min + alpha * 2 * (rho_mean - rho_min))
        if alpha > 0.5:
            return (2 * rho_mean - rho_max) + alpha * 2 * (rho_max - rho_mean)

    # ------------------------------------------------------------ the device path
    def _buffers(self):
        if self._buf is None:
            ph = self.ph_object
            f64, dev = torch.float64, ph.device
            nns = max(ph.NNS, 1)
            self._buf = {
                "stats": torch.zeros(4 * nns, dtype=f64, device=dev),
                "partial": torch.zeros(2 * max(int(ph._tree.npart), 1), dtype=f64, device=dev),
                "scen_denom": torch.zeros(max(ph._S, 1), dtype=f64, device=dev),
                "denom": torch.zeros(nns + 1, dtype=f64, device=dev),
                "rho_node": torch.zeros(nns, dtype=f64, device=dev),
                "kept": torch.zeros(nns, dtype=torch.int32, device=dev),
            }
            self.kept = self._buf["kept"]
        return self._buf

    def compute_rho_device(self, cost_t, indep_denom=False, install=True):
        """The rule for every (node, slot) entry of any tree, on the device.

        cost_t: [N][S] device tensor of costs (any sign; the rule takes |cost|).
        Returns the [NNS] tensor of per-entry rho; ``self.kept`` ([NNS] int32)
        marks the entries whose rho was not finite and stayed as it was.  With
        ``install`` the scenarios' rho is overwritten (and the next solve picks
        it up); without, a scratch copy takes the writes.  No host read."""
        ph = self.ph_object
        alpha = float(cfg_get(self.cfg, "order_stat"))
        assert alpha != -1.0, "you need to set the order statistic parameter for rho using --order-stat"
        assert (alpha >= 0 and alpha <= 1), "0 is the min, 0.5 the average, 1 the max"
        b = self._buffers()
        NNS = ph.NNS
        if NNS == 0 or ph.batch.nonant.N == 0:
            return b["rho_node"][:0]
        assert cost_t.numel() == ph.batch.nonant.N * ph._S and cost_t.dtype == torch.float64
        cost_t = cost_t.contiguous()
        lib = ph._native
        denom = self._grad_denom_device() if indep_denom else None
        ph._settle()
        lib.check(ph._ctx, lib.cost_rho_stats(ph._ctx, ctypes.byref(ph._tree), cost_t.data_ptr(), ph._x.data_ptr(),
                                              ph._xbar_node.data_ptr(), ph._xbar_idx_t.data_ptr(),
                                              denom.data_ptr() if denom is not None else None,
                                              b["partial"].data_ptr(), b["scen_denom"].data_ptr(),
                                              b["stats"].data_ptr(), ph._stream()), "cost_rho_stats")
        ph.mpicomm.allreduce_(b["stats"][:2 * NNS])
        ph.mpicomm.allreduce_max_(b["stats"][2 * NNS:4 * NNS])
        opts = _native.CostRhoOpts()
        opts.order_stat = alpha
        rho = ph._rho if install else ph._rho.clone()
        lib.check(ph._ctx, lib.cost_rho_apply(ph._ctx, ctypes.byref(ph._tree), ctypes.byref(opts),
                                              b["stats"].data_ptr(), ph._xbar_idx_t.data_ptr(), rho.data_ptr(),
                                              b["rho_node"].data_ptr(), b["kept"].data_ptr(), ph._stream()),
                  "cost_rho_apply")
        if install:
            ph._bump()
        return b["rho_node"][:NNS]

    def _cost_tensor(self):
        """[N][S] device tensor of self.c for the local scenarios."""
        ph = self.ph_object
        names = ph.batch.nonant.var_names
        cost = np.array([[self.c[(sname, vname)] for sname in ph.local_scenario_names] for vname in names],
                        dtype=np.float64).reshape(len(names), ph._S)
        return torch.as_tensor(cost).to(ph.device)

    def compute_rho(self, indep_denom=False):
        """rhos for each variable using the WW heuristic.

        Returns:
           rho (dict): {variable name: rho} on cylinder rank 0, None elsewhere
        """
        ph = self.ph_object
        assert not ph.multistage, "compute rho only works for two stage for now"
        rho_node = self.compute_rho_device(self._cost_tensor(), indep_denom=indep_denom, install=False)
        if ph.cylinder_rank == 0:
            vals = rho_node.cpu().numpy()
            nn = ph.batch.nonant
            return {nn.var_names[j]: float(vals[int(nn.slot_local[j])]) for j in range(nn.N)}

    def write_rho(self):
        """Write the computed rhos in the file --rho-file."""
        rho_file = cfg_get(self.cfg, "rho_file")
        if rho_file == '':
            pass
        else:
            rho_data = self.compute_rho()
            if self.ph_object.cylinder_rank == 0:
                with open(rho_file, 'w') as file:
                    writer = csv.writer(file)
                    writer.writerow(['#Rho values'])
                    for (vname, rho) in rho_data.items():
                        writer.writerow([vname, rho])


def _find_var(scenario, fullname):
    """The variable called fullname of a scenario model or scenario view: (id, found)."""
    if hasattr(scenario, "find_component"):
        vo = scenario.find_component(fullname)
        return (id(vo), True) if vo is not None else (None, False)
    for v in getattr(scenario, "_vars", ()):                     # a LinearModel
        if v.name == fullname:
            return id(v), True
    data = getattr(scenario, "_mpisppy_data", None)
    if data is not None and hasattr(data, "nonant_indices"):     # a view: no model variables to take id() of
        for v in data.nonant_indices.values():
            if v.name == fullname:
                return getattr(v, "varid", id(v)), True
    return None, False


class Set_Rho():
    """Interface to set the computed rhos in PH.

    Args:
       cfg: config object (rho_path: the rho csv file)
    """
    def __init__(self, cfg):
        self.cfg = cfg

    def rho_setter(self, scenario):
        """rho setter to be used in the PH algorithm

        Returns:
           rho_list (list): list of (id(variable), rho)
        """
        assert self.cfg is not None, "you have to give the rho_setter a cfg"
        rhofile = cfg_get(self.cfg, "rho_path")
        assert rhofile != '', "use --rho-path to give the path of your rhos file"
        rho_list = list()
        with open(rhofile) as infile:
            reader = csv.reader(infile)
            for row in reader:
                if not row or row[0].startswith('#'):
                    continue
                fullname = row[0]
                vid, found = _find_var(scenario, fullname)
                if found:
                    rho_list.append((vid, float(row[1])))
                else:
                    raise RuntimeError(f"rho values from {rhofile} found Var {fullname} "
                                       f"that is not found in the scenario given "
                                       f"(name={getattr(scenario, 'name', None)})")
        return rho_list
