"""``model_utils`` of the reference (/root/reference/model_utils.py: featurize :19-125, loss_nll :128, loss_smoothed :140, the training
ProteinMPNN :396-470, NoamOpt :474, get_std_opt :509) -> thermompnn_amd."""
import _repo  # noqa: F401
from thermompnn_amd.model_utils import NoamOpt, ProteinMPNN, featurize, get_std_opt, loss_nll, loss_smoothed  # noqa: F401
