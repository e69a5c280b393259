"""XhatSpecific: try the scenarios named in
``options["xhat_specific_options"]["xhat_scenario_dict"]`` ({node name:
scenario name}) as xhat (extensions/xhatspecific.py:9-84).

Options (``xhat_specific_options``): ``xhat_scenario_dict``,
``xhat_solver_options``, ``keep_solution`` (default True), ``csvname``,
``dump_prefix``.  As a PH extension it acts in ``post_everything`` only, so the
PH iterations keep running in the device loop.
"""
from .xhatbase import XhatBase


class XhatSpecific(XhatBase):
    def __init__(self, spo):
        super().__init__(spo)
        self.options = spo.options["xhat_specific_options"]
        self.solver_options = self.options["xhat_solver_options"]
        self.keep_solution = not ("keep_solution" in self.options and not self.options["keep_solution"])

    def xhat_tryit(self, xhat_scenario_dict, verbose=False, restore_nonants=True):
        """E[obj] with every nonant fixed at the named scenarios' cached values,
        or None if that is infeasible (xhatspecific.py:24-59)."""
        def _vb(msg):
            if verbose and self.cylinder_rank == 0:
                print("  xhat_specific: " + msg)
        _vb("Enter XhatSpecific.xhat_tryit to try: " + str(xhat_scenario_dict))
        _vb("   Solver options=" + str(self.solver_options))
        obj = self._try_one(xhat_scenario_dict, solver_options=self.solver_options, verbose=False,
                            restore_nonants=restore_nonants)
        _vb("Infeasible" if obj is None else "Feasible, returning " + str(obj))
        return obj

    def post_everything(self):
        # if we're keeping the solution, we *do not* restore the nonants
        restore_nonants = not self.keep_solution
        self.opt.disable_W_and_prox()
        xhat_scenario_dict = self.options["xhat_scenario_dict"]
        # the donors' values are the scenarios' current ones (the reference's
        # _try_one saves them itself, xhatbase.py:62)
        self.opt._save_nonants()
        obj = self.xhat_tryit(xhat_scenario_dict, verbose=self.verbose, restore_nonants=restore_nonants)
        self.opt.reenable_W_and_prox()
        # to make available to tester
        self._xhat_specific_obj_final = obj
        self.xhat_common_post_everything("xhat specified scenario", obj, xhat_scenario_dict, restore_nonants)
