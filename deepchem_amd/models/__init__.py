from deepchem_amd.models.models import Model
from deepchem_amd.models import losses, optimizers, torch_models
from deepchem_amd.models.torch_models import AtomConvModel, CGCNN, CGCNNModel, DMPNNModel, DTNNModel, GraphConvModel, LCNN, LCNNModel, MATModel, MEGNetModel, TorchModel, WeaveModel
from deepchem_amd.models.callbacks import ValidationCallback
