from deepchem_amd.utils.batch_utils import batch_coulomb_matrix_features  # noqa: F401
