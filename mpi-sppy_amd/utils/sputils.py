"""Scenario-tree utilities used on the PH path.

Restatements of the reference helpers in ``mpisppy/utils/sputils.py``:
``extract_num`` (481-490), ``node_idx`` (492-519), ``parent_ndn`` (544-548),
``create_nodenames_from_branching_factors`` (934-959), ``attach_root_node``
(844-860) and the contiguous rank-slicing rule of
``_ScenTree.scen_names_to_ranks`` (774-840, slices at 803-810).
"""
import re

import numpy as np

from ..scenario_tree import ScenarioNode


def extract_num(string):
    return int(re.compile(r"(\d+)$").search(string).group(1))


def _nodenum_before_stage(t, branching_factors):
    return int(sum(np.prod(branching_factors[0:i]) for i in range(t)))


def node_idx(node_path, branching_factors):
    if node_path == []:
        return 0
    stage_id = 0
    for t in range(len(node_path)):
        stage_id = node_path[t] + branching_factors[t] * stage_id
    return _nodenum_before_stage(len(node_path), branching_factors) + stage_id


def parent_ndn(nodename):
    if nodename == "ROOT":
        return None
    return re.search(r"(.+)_(\d+)", nodename).group(1)


def create_nodenames_from_branching_factors(BFS):
    stage_nodes = ["ROOT"]
    nodenames = ["ROOT"]
    if len(BFS) == 1:
        return nodenames
    for bf in BFS:
        old = stage_nodes
        stage_nodes = []
        for k in range(len(old)):
            stage_nodes += ["%s_%i" % (old[k], b) for b in range(bf)]
        nodenames += stage_nodes
    return nodenames


def rank_slices(scen_count, n_proc):
    """rank -> list of scenario indices; contiguous, ``int(r*S/R)`` boundaries."""
    if n_proc == 1:
        return [list(range(scen_count))]
    avg = scen_count / n_proc
    return [list(range(int(i * avg), int((i + 1) * avg))) for i in range(n_proc)]


def rank_bounds(scen_count, n_proc):
    """[(first, last+1)] per rank, same rule as :func:`rank_slices`."""
    if n_proc == 1:
        return [(0, scen_count)]
    avg = scen_count / n_proc
    return [(int(i * avg), int((i + 1) * avg)) for i in range(n_proc)]


def attach_root_node(model, firstobj, varlist, nonant_ef_suppl_list=None):
    model._mpisppy_node_list = [
        ScenarioNode("ROOT", 1.0, 1, firstobj, varlist, model,
                     nonant_ef_suppl_list=nonant_ef_suppl_list)
    ]


class TreeNode:
    """A scenario-tree node as the reference's ``_TreeNode`` exposes it
    (sputils.py:675-724): ``name``, ``stage`` (1-based), ``kids``, ``is_leaf``
    and the indices ``scenfirst`` .. ``scenlast`` (inclusive) of its scenarios
    in ``all_scenario_names``."""

    def __init__(self, name, stage, scenfirst, scenlast, is_leaf=False):
        self.name = name
        self.stage = stage
        self.scenfirst = scenfirst
        self.scenlast = scenlast
        self.is_leaf = is_leaf
        self.kids = []

    def __repr__(self):
        return "TreeNode(%s, scenarios %d..%d)" % (self.name, self.scenfirst, self.scenlast)


def nonleaf_tree_nodes(all_nodenames, scen_count):
    """{name: TreeNode} of the non-leaf nodes, ROOT first and depth first as
    the reference's ``_ScenTree.nonleaves`` (sputils.py:755-763).  Scenarios are
    the leaves in depth-first order (children by their number), one per leaf;
    a two-stage tree (``["ROOT"]``) has no leaf nodes and ROOT owns every
    scenario."""
    if all_nodenames is None or list(all_nodenames) == ["ROOT"]:
        return {"ROOT": TreeNode("ROOT", 1, 0, scen_count - 1)}
    names = set(all_nodenames)
    out = {}

    def make(name, stage, first):
        k = 0
        kids = []
        nxt = first
        while "%s_%d" % (name, k) in names:
            kid = make("%s_%d" % (name, k), stage + 1, nxt)
            nxt = kid.scenlast + 1
            kids.append(kid)
            k += 1
        if not kids:
            return TreeNode(name, stage, first, first, is_leaf=True)
        node = TreeNode(name, stage, first, nxt - 1)
        node.kids = kids
        return node

    def collect(node):
        if node.is_leaf:
            return
        out[node.name] = node
        for kid in node.kids:
            collect(kid)

    collect(make("ROOT", 1, 0))
    return out


def find_leaves(all_nodenames):
    if all_nodenames is None or all_nodenames == ["ROOT"]:
        return {"ROOT": False}
    s = set(all_nodenames)
    return {ndn: (ndn + "_0") not in s for ndn in all_nodenames}
