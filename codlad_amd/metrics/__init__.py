"""The evaluation and structure-analysis entry points, one module per concern; every public name is read from here
(`from codlad_amd import metrics; metrics.X`).  recon: the reference's test-loop metrics; ensemble: superposed RMSD and
diversity; geometry, stereo: the reference-free checks; relax: the clash relaxation; observables: SASA, Rg, contact maps;
dssp: secondary structure; saxs: scattering profiles; pair_distribution: typed pair-distance histograms, P(r) and the
profiles made from them; reweight: maximum-entropy weights against data; cluster: the all-pairs RMSD matrix of a pool and
Daura's clustering; pca: the mean structure after mutual superposition, RMSF, covariance and principal components; compare: distance,
torsion, Rg and cluster-population divergences of two ensembles; lddt: the local distance difference test against the true
frames; polymer: the chain statistics of a disordered ensemble - hydrodynamic radius, gyration-tensor shape, end-to-end
distance, internal distance scaling and its Flory exponent; drmsd: the superposition-free distance RMSD of every pair of a
pool or of two pools, of a list of pairs, and Daura's clustering at a dRMSD cut-off; torsion: the ensemble in its torsion
angles - (cos, sin) features, circular statistics, dihedral PCA, the torsion distance of every pair and Daura's clustering
at a torsion cut-off; _inputs: what they share."""
from .. import _lib   # noqa: F401
from ._inputs import COV_CUTOFF, exclusion_csr   # noqa: F401
from .recon import *   # noqa: F401,F403 (every public name of a module, C and torch among them as in the module this replaced)
from .ensemble import *   # noqa: F401,F403
from .ensemble import _moments, _selection   # noqa: F401 (the tests reach these six)
from .geometry import *   # noqa: F401,F403
from .stereo import *   # noqa: F401,F403
from .relax import *   # noqa: F401,F403
from .relax import _relax_table_args, _relax_tables_on   # noqa: F401
from .observables import *   # noqa: F401,F403
from .observables import _res_table, _sasa_atom_tables   # noqa: F401
from .dssp import *   # noqa: F401,F403
from .saxs import *   # noqa: F401,F403
from .saxs import _saxs_tables   # noqa: F401
from .pair_distribution import *   # noqa: F401,F403 (pair_distribution the function takes the module's name here)
from .reweight import *   # noqa: F401,F403
from .cluster import *   # noqa: F401,F403
from .pca import *   # noqa: F401,F403 (pca the function takes the module's name here)
from .compare import *   # noqa: F401,F403
from .lddt import *   # noqa: F401,F403 (lddt the function takes the module's name here)
from .polymer import *   # noqa: F401,F403
from .drmsd import *   # noqa: F401,F403
from .torsion import *   # noqa: F401,F403
