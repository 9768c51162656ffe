from deepchem_amd.feat import mol_graphs
from deepchem_amd.feat.mol_graphs import ConvMol, MultiConvMol
from deepchem_amd.feat import graph_features
from deepchem_amd.feat.graph_features import ConvMolFeaturizer, WeaveFeaturizer
from deepchem_amd.feat.graph_features import NativeGraphFeaturizer
from deepchem_amd.feat.graph_data import GraphData
from deepchem_amd.feat.mat_featurizer import MATEncoding, MATFeaturizer
