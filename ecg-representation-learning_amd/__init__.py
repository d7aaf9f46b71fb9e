"""
ecg_representation_learning_amd -- MI355X-native (gfx950) drop-in for the ECG-ViT train step of
StefanHeng/ECG-Representation-Learning (`ecg_transformer.models`): same `EcgVitConfig` / `EcgVit.forward ->
ModelOutput(loss, logits)` / train-step surface, executed by hand-written HIP kernels behind a C-ABI
(`include/ecgvit_hip.h`, `csrc/`).  Importing the package never needs a GPU; running the model does, and
fails loudly when the HIP library is absent (no CPU / eager fallback by design).
"""
from .check_args import ca, CheckArg
from .ecg_vit import EcgVitConfig, EcgVit, ModelOutput, RolloutOutput, HipViT, MaskedEcgVit, load_trained
from .train import get_train_args, lr_multiplier, HipTrainStep, HipProbeStep, clip_grad_norm_
from .transform import FusedInputTransform, fit_dynamic_normalize, DynamicNormalizeFit
from .tokenizer import EcgTokenizer, KMeansPlusPlus, ScalableKMeansPlusPlus, Dbscan
from .denoise import EcgDenoiser, design_lowpass, rloess, lowpass, estimate_noise_std, nlm
from . import denoise
from .resample import resample, resampled_length, plan as resample_plan, chirp_length as resample_chirp_length, route as resample_route
from .metrics import get_accuracy, eval_counts, HipEvaluator, HipEncoder, HipRollout, HipKnnProbe
from .knn import KnnIndex, knn_search, knn_merge
from . import knn
from .rank_metrics import rank_scores, auroc_counts, bootstrap_auc, RankedScores, BootstrapResult
from . import rank_metrics
from .pr_metrics import pr_walk, pr_counts, bootstrap_pr, paired_diff_ci, PrCounts, PrBootstrapResult
from . import pr_metrics
from .feed import DeviceFeeder, RaggedDeviceFeeder, ptbxl_splits, lbs2multi_hot, open_records
from . import hip
from . import ddp
from . import workload

__all__ = ['ca', 'CheckArg', 'EcgVitConfig', 'EcgVit', 'ModelOutput', 'RolloutOutput', 'HipViT', 'MaskedEcgVit', 'load_trained', 'get_train_args', 'lr_multiplier',
           'HipTrainStep', 'HipProbeStep', 'clip_grad_norm_', 'FusedInputTransform', 'fit_dynamic_normalize', 'DynamicNormalizeFit', 'EcgTokenizer', 'KMeansPlusPlus', 'ScalableKMeansPlusPlus', 'Dbscan', 'EcgDenoiser', 'design_lowpass', 'rloess', 'lowpass', 'estimate_noise_std', 'nlm', 'denoise', 'resample', 'resampled_length', 'resample_plan', 'resample_chirp_length', 'resample_route', 'get_accuracy', 'eval_counts', 'HipEvaluator', 'HipEncoder', 'HipRollout', 'HipKnnProbe', 'KnnIndex', 'knn_search', 'knn_merge', 'knn', 'rank_scores', 'auroc_counts', 'bootstrap_auc', 'RankedScores', 'BootstrapResult', 'rank_metrics', 'DeviceFeeder', 'RaggedDeviceFeeder', 'ptbxl_splits', 'lbs2multi_hot', 'open_records', 'hip', 'ddp', 'workload', 'pr_walk', 'pr_counts', 'bootstrap_pr', 'paired_diff_ci', 'PrCounts', 'PrBootstrapResult', 'pr_metrics']
