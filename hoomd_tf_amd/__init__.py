"""hoomd_tf_amd -- MI355X-native drop-in for hoomd-tf's per-particle force/energy path.

Mirrors the reference's Python surface for that path (``hoomd.htf``): ``SimModel``,
``tfcompute``, ``compute_nlist_forces``, ``nlist_rinv``, ``safe_norm``,
``RBFExpansion``, ``WCARepulsion``, ``EDSLayer`` ...  All arithmetic runs in the
hand-written HIP kernels of ``libhtf_amd.so`` (C ABI: include/htf_amd.h; the coarse-grained mapping ops
``center_of_mass`` / ``compute_nlist``: include/htf_cg.h; the molecular geometry ops ``mol_bond_distance`` / ``mol_angle`` /
``mol_dihedral``: include/htf_geom.h; the cell-binned route of ``compute_nlist``: include/htf_nlist.h; the descriptor
network ``DescriptorMLP``, its force-matching sweep, smooth cutoff and one network per particle species: include/htf_bp.h; its conservative forces ``F = -d(sum_i E_i)/dr``,
``DescriptorMLP(conservative=True)``, and the slot-aligned index tensor ``Nlist.index`` they read: include/htf_cforce.h; force
matching on those forces, ``DescriptorMLP(trainable="total")`` and ``total_loss_gradient``: include/htf_ctrain.h; angular channels on the conservative
forces, ``DescriptorMLP(conservative=True, l_max=1 or 2)``: include/htf_angular.h; force matching on those, ``DescriptorMLP(l_max=1 or 2,
trainable="angular")`` and ``angular_loss_gradient``: include/htf_atrain.h; the same forces and sweeps on one slab domain's
rows, with the ghost particles' table rows from their owners: include/htf_cghost.h; a committee of M such networks,
``DescriptorMLP(conservative=True, n_models=M)``, whose ``total_forces`` gives the mean-model forces and leaves the per-particle
model deviation in ``layer.deviation``, the descriptor and every exponential formed once for all members: include/htf_committee.h;
``trainable="committee"`` trains that committee where it runs, ``committee_loss_gradient`` being the force-matching sweep of all
M members at once, one wave per member on the same rows: include/htf_cmt_train.h).
The offline path ``iter_from_trajectory`` / ``ArrayTrajectory`` runs a
``SimModel`` over stored frames.
``DeviationSelector`` consumes the committee's deviation where it is produced: ``sel.update(layer.deviation, positions, box)``
classifies the frame by its largest deviation (accurate, candidate, failed: the DP-GEN rule) and keeps the candidates'
positions and box in a fixed-capacity device buffer, in three launches and without a read-back; ``sel.trajectory()`` hands
them to ``iter_from_trajectory`` for labelling and offline training (include/htf_select.h).
"""
from . import _lib
from ._lib import NlistOverflowError, SkewedBoxError
from . import ops
from .ops import Potential, Context
from . import standin
from .simmodel import (SimModel, compute_nlist_forces, compute_positions_forces, nlist_rinv, safe_norm,
                       box_size, wrap_vector, compute_rdf, masked_nlist, reduce_sum, pairwise_unit_forces, Nlist,
                       norm, cast, divide_no_nan, Positions, sort, exp, log, tanh, sqrt, square, pow, abs, minimum, maximum, where,
                       gather, equal, not_equal, erf, erfc, sigmoid, softplus, sin, cos,
                       MolSimModel, find_molecules, MeanTensor)
from .layers import RBFExpansion, WCARepulsion, EDSLayer, PairMLP, SoftRDFCV, LJLayer, Dense, DescriptorMLP
from . import optimizers
from .cgmap import sparse_mapping, center_of_mass, compute_nlist
from .molgeom import mol_bond_distance, mol_angle, mol_dihedral, mol_features_multiple
from .tensorflowcompute import tfcompute
from .trajectory import ArrayTrajectory, iter_from_trajectory
from .select import DeviationSelector

__version__ = "0.1.0"
