"""XhatLooper: try the first ``scen_limit`` scenarios as xhat, one after the
other, and keep the best (extensions/xhatlooper.py:9-130).

One difference from the reference, on purpose: its loop stops at the first
feasible scenario (:88-90); a trial here is one batched solve on the device, so
every one of the ``scen_limit`` scenarios is tried and the best objective is
returned (with ``restore_nonants=False`` the nonants are left fixed at that
best candidate).

Options (``xhat_looper_options``): ``scen_limit``, ``xhat_solver_options``,
``keep_solution`` (default True), ``csvname``, ``dump_prefix``,
``append_file_name``.  Two-stage problems only, as the reference.
"""
from .xhatbase import XhatBase


class XhatLooper(XhatBase):
    def __init__(self, ph):
        super().__init__(ph)
        self.options = ph.options["xhat_looper_options"]
        self.solver_options = self.options["xhat_solver_options"]
        self._xhat_looper_obj_final = None
        self.keep_solution = not ("keep_solution" in self.options and not self.options["keep_solution"])

    def xhat_looper(self, scen_limit=1, seed=None, verbose=False, restore_nonants=True):
        """Try scenarios 0 .. scen_limit-1 of ``all_scenario_names`` as the ROOT
        donor; returns (objective, {"ROOT": scenario name}) of the best feasible
        one, or (None, the last dict tried) (xhatlooper.py:25-101)."""
        def _vb(msg):
            if verbose and self.cylinder_rank == 0:
                print("    rank {} xhat_looper: {}".format(self.cylinder_rank, msg))
        if self.opt.multistage:
            raise RuntimeError("xhatlooper cannot do multi-stage")
        if seed is not None:
            raise RuntimeError("xhat_looper: a seeded (random) scenario order is not implemented")
        obj = None
        snamedict = None
        nscen = len(self.opt.all_scenario_names)
        llim = min(scen_limit, nscen)
        _vb("Enter xhat_looper to try " + str(llim) + " scenarios.")
        self.opt._save_nonants()      # to cache for use in fixing
        better = (lambda a, b: a < b) if self.opt.is_minimizing else (lambda a, b: a > b)
        last = None
        for snum in range(llim):
            sname = self.opt.all_scenario_names[snum]
            _vb("Trying scenario " + sname)
            last = {"ROOT": sname}
            val = self._try_one(last, solver_options=self.solver_options, verbose=False, restore_nonants=True)
            if val is None:
                _vb("    Infeasible")
            else:
                _vb("    Feasible, " + str(val))
                if obj is None or better(val, obj):
                    obj, snamedict = val, last
        if obj is None:
            snamedict = last
        elif not restore_nonants:
            # leave the nonants fixed at the best candidate
            obj = self._try_one(snamedict, solver_options=self.solver_options, verbose=False, restore_nonants=False)
        if "append_file_name" in self.options and self.opt.cylinder_rank == 0:
            with open(self.options["append_file_name"], "a") as f:
                f.write(", " + str(obj))
        self.xhatlooper_obj = obj
        return obj, snamedict

    def pre_iter0(self):
        if self.opt.multistage:
            raise RuntimeError("xhatlooper cannot do multi-stage")

    def post_everything(self):
        restore_nonants = not self.keep_solution
        self.opt.disable_W_and_prox()
        obj, snamedict = self.xhat_looper(scen_limit=self.options["scen_limit"], verbose=self.verbose,
                                          restore_nonants=restore_nonants)
        self.opt.reenable_W_and_prox()
        # "secret menu" way to see the value in a script
        self._xhat_looper_obj_final = obj
        self.xhat_common_post_everything("xhatlooper", obj, snamedict, restore_nonants)
