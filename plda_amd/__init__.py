"""plda_amd -- MI355X (gfx950) native PLDA engine behind the `liblda.PLDA` API.

Layout (only what the hot path needs):
  csrc/       hand-written HIP kernels + the C ABI (include/plda_hip.h)
  lib/        built libplda_hip.so (in-tree, git-ignored)
  _native.py  ctypes binding of the C ABI (fails loudly if the .so or a GPU is missing)
  libplda.py  `MPlda`: counterpart of the reference's CPython type libplda.MPlda
  cosine.py   `Cosine`: the cosine back-end behind MPlda's scoring interface (csrc/cosine.hip)
  sharding.py row-sharded trials matrix across ranks (torch.distributed / RCCL)
  calibration.py linear score calibration, Cllr, actual DCF (csrc/calib.hip)
  fusion.py   linear fusion of K systems' scores by logistic regression (csrc/fusion.hip)
  adaptation.py the result of MPlda.adapt: unsupervised PLDA domain adaptation and model interpolation (csrc/adapt.hip)
  identify.py rank-N identification rates and the CMC curve from the ids of MPlda.top_n (csrc/topn.hip); pure NumPy
  diarize.py  speaker clustering: batched average-linkage AHC on score blocks (csrc/ahc.hip), cut() in pure NumPy; VBx resegmentation (csrc/vbx.hip); dense scoring in every recording's PCA subspace (csrc/dense_pca.hip)
  der.py      diarisation error rate under the optimal speaker mapping, and the sweep of one merge record over thresholds (csrc/der.hip)
              and its time-based form: overlapped reference speech, collar, UEM (csrc/der_time.hip)
  trialkey.py trial keys: which pairs are trials and their condition buckets, the per-(bucket, class) score lists on the device and per-condition metrics (csrc/partition.hip)
  rttm.py     RTTM files and per-segment reference labels from reference turns; pure Python / NumPy
"""
from .libplda import MPlda  # noqa: F401
from .cosine import Cosine  # noqa: F401
from . import calibration  # noqa: F401
from . import fusion  # noqa: F401
from . import identify  # noqa: F401
from . import adaptation  # noqa: F401
from . import diarize  # noqa: F401
from . import der  # noqa: F401
from . import rttm  # noqa: F401
from . import trialkey  # noqa: F401
from .calibration import Calibration  # noqa: F401
from .fusion import Fusion  # noqa: F401
from .adaptation import Adaptation  # noqa: F401
from .trialkey import TrialKey  # noqa: F401

__all__ = ["MPlda", "Cosine", "Calibration", "Fusion", "Adaptation", "TrialKey", "trialkey", "calibration", "fusion", "identify", "adaptation", "diarize", "der", "rttm"]
