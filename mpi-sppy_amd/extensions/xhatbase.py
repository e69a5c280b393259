"""XhatBase: try the nonants of one donor scenario per tree node as the
incumbent (extensions/xhatbase.py:14-312), the base of XhatSpecific,
XhatLooper and the xhatshuffle spoke.

A trial is: donor table -> ``phx_donor_gather`` on the device copy of the
nonant cache -> one SUM all-reduce of the [NNS] node-slot vector (exactly one
rank contributes per node, so every rank receives the donor's bits: the
reference's per-node ``bcast``, :79-123) -> ``phx_fix_nonants`` (lb = ub = value
on the device, the same values into x) -> one batched solve on the
fixed-nonant lane module -> ``infeas_prob`` / ``Eobjective``.  Nothing is
copied to the host but the scalars those two read, and no bound array is
uploaded.

Differences from the reference, on purpose:
  * the reference's ``_try_one`` begins with ``_save_nonants()`` (:62).  After a
    feasible trial with ``restore_nonants=False`` that overwrites every
    scenario's cache with the candidate just tried, so every later donor
    repeats it until the hub sends new nonants.  Here donors are always read
    from the nonant cache last set by ``_save_nonants`` / ``_put_nonant_cache``
    (kept as a device [N][S] copy beside the host one, uploaded only when it
    changes; ``_try_one`` saves only when there is no cache yet): the first
    trial after each hub update is the reference's, the following ones are
    real new candidates.  The callers that want the current values as donors
    (XhatLooper, XhatSpecific as PH extensions) save them first, as the
    reference's xhat_looper does (:71 of xhatlooper.py);
  * ``scenario_name_to_rank`` holds cylinder ranks (every node's comm is the
    cylinder's here, see SPBase);
  * ``stage2EFsolvern`` is not supported (NotImplementedError): it builds an
    extensive form per second-stage node with an external solver;
  * bundles and linearised prox terms are rejected, as the reference rejects
    bundles for its xhat spokes.
"""
import numpy as np

from .extension import Extension


class XhatBase(Extension):
    def __init__(self, opt):
        super().__init__(opt)
        self.cylinder_rank = self.opt.cylinder_rank
        self.n_proc = self.opt.n_proc
        self.verbose = self.opt.options["verbose"]
        self.scenario_name_to_rank = opt.scenario_names_to_rank

    # ------------------------------------------------------------ the trial
    def _donor_table(self, snamedict):
        """int32 [local nodes]: the donor's local scenario index per local tree
        node, -1 when it lives on another rank; the reference's checks."""
        opt = self.opt
        lo, hi = opt._local_lo, opt._local_hi
        index = getattr(self, "_sname_index", None)
        if index is None:
            index = self._sname_index = {nm: k for k, nm in enumerate(opt.all_scenario_names)}
        local_nodes = sorted(set(t[0] for t in opt._tiles))
        donor = np.full(len(local_nodes), -1, dtype=np.int32)
        if len(snamedict) == 1:
            snamedict["ROOT"]      # also serves as an assert (xhatbase.py:74)
        for k, v in enumerate(local_nodes):
            ndn = opt._node_names[v]
            if ndn not in snamedict:
                raise RuntimeError(f"{ndn} not in snamedict={snamedict}")
            sname = snamedict[ndn]
            if sname not in self.scenario_name_to_rank[ndn]:
                print(f"For ndn={ndn}, snamedict[ndn] not in self.scenario_name_to_rank[ndn]")
                print(f"snamedict[ndn]={sname}")
                raise RuntimeError("Bad scenario selection for xhat")
            g = index[sname]
            if lo <= g < hi:
                donor[k] = g - lo
        return donor

    def _try_one(self, snamedict, solver_options=None, verbose=False, restore_nonants=True,
                 stage2EFsolvern=None, branching_factors=None):
        """Fix every scenario's nonants at the values the scenarios named in
        ``snamedict`` ({non-leaf node name: scenario name}) hold in the nonant
        cache, solve, and return E[obj], or None when some scenario is
        infeasible (the nonants are restored then).  ``restore_nonants``: put
        values and fixedness back after a feasible trial too; False leaves the
        nonants fixed at the candidate (xhatbase.py:38-229)."""
        opt = self.opt
        if stage2EFsolvern is not None:
            raise NotImplementedError("stage2EFsolvern: the per-node extensive forms of the reference's _try_one "
                                      "need an external EF solver; the engine evaluates candidates by batched "
                                      "scenario solves only")
        if opt._bundles is not None or opt._prox_lin is not None:
            raise RuntimeError("xhat trials cannot be combined with bundles or linearised prox terms")
        sopt = solver_options
        if solver_options is not None and "Tee" in solver_options:
            sopt = dict(solver_options)
            del sopt["Tee"]
        donor = self._donor_table(snamedict)
        if getattr(opt, "nonant_cache", None) is None:
            opt._save_nonants()
        opt._fix_nonants_device(opt._donor_values(donor))
        opt.solve_loop(solver_options=sopt, verbose=verbose, tee=False)
        infeasP = opt.infeas_prob()
        if infeasP != 0.:
            # restoring does no harm if this solution is infeasible
            opt._restore_nonants_device()
            return None
        if verbose and self.cylinder_rank == 0:
            print("   Feasible xhat found:", snamedict)
        obj = opt.Eobjective(verbose=verbose)
        if restore_nonants:
            opt._restore_nonants_device()
        return obj

    # ------------------------------------------------------------ reporting
    def csv_nonants(self, snamedict, fname):
        """The donors' nonants of each node as ``fname_<node>_<scenario>.csv``,
        written by the rank that holds the scenario (xhatbase.py:232-253)."""
        opt = self.opt
        nn = opt.batch.nonant
        vals = None
        for ndn, sname in snamedict.items():
            if sname not in opt.local_scenario_names:
                continue
            if vals is None:
                vals = opt.nonant_values()
            s = opt.local_scenario_names.index(sname)
            stage = ndn.count("_") + 1
            with open(fname + "_" + ndn + "_" + sname + ".csv", "w") as f:
                f.write(ndn)
                for j in np.nonzero(nn.slot_stage == stage)[0]:
                    f.write(', "' + str(nn.var_names[j]) + '", ' + str(float(vals[s, j])))
                f.write("\n")

    def xhat_common_post_everything(self, extname, obj, snamedict, restored_nonants):
        """What the xhat extensions' post_everything share (xhatbase.py:282-308)."""
        if (obj is not None) and (not restored_nonants):
            self.opt.tree_solution_available = True
            self.opt.first_stage_solution_available = True
        if (obj is not None) and (self.opt.spcomm is not None):
            self.opt.spcomm.BestInnerBound = self.opt.spcomm.InnerBoundUpdate(obj, char="E")
        if self.cylinder_rank == 0 and self.verbose:
            print("****", extname, "Used scenarios", str(snamedict), "to get xhat Eobj=", obj)
        if "csvname" in self.options:
            self.csv_nonants(snamedict, self.options["csvname"])
        if "dump_prefix" in self.options:
            self.csv_nonants(snamedict, self.options["dump_prefix"] + "_nonant_" + extname)

    def post_iter0(self):
        self.comms = self.opt.comms
