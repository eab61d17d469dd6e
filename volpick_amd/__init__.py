"""volpick_amd — MI355X-native sliding-window phase picking with the volpick weights.

Drop-in for the ``seisbench.models`` picker API volpick users call:

    import volpick_amd as sbm
    picker = sbm.EQTransformer.from_pretrained("volpick")
    picks = picker.classify(stream, batch_size=256, overlap=5500, blinding=(500, 500),
                            stacking="avg", P_threshold=0.2, S_threshold=0.2).picks

``volpick_amd.spectrogram`` is the module of the reference's ``spectrogram()`` as numbers on the GPU:
``volpick_amd.spectrogram.spectrogram(x, samp_rate, ...)`` for a CUDA tensor ``(..., N)``, ``Trace.spectrogram()`` /
``Stream.spectrogram()`` for traces (device-backed ones stay on the device), ``volpick_amd.spectrogram.plan`` for the host
plan, ``release_spectrogram_scratch`` for the scratch the kernel keeps.
"""
from .models import EQTransformer, PhaseNet, WaveformModel  # noqa: F401
from .picks import ClassifyOutput, Detection, DetectionList, Pick, PickList  # noqa: F401
from .stream import Stream, Trace, UTCDateTime, pinned_array, to_device  # noqa: F401
from ._lib import VolpickHipError  # noqa: F401
from .io import plan_file_blocks, read, read_many, scan_segments, write_mseed  # noqa: F401
from .files import classify_files  # noqa: F401
from .convert import bank_from_mseed, bank_from_streams, plan_event  # noqa: F401
from .attributes import bank_attributes, pick_attributes, plan_rows  # noqa: F401
from .signal import butter_sos, detrend_array, detrend_device, filter_array, sos_filter_device  # noqa: F401
from .evaluate import (eval_task0, opt_prob_metrics, sweep_bank, sweep_windows, task0_counts, task0_metrics,  # noqa: F401
                       task0_residuals, task0_tnr, task0_truth)
from .train import EQTransformerLit, bce_loss, validate_batches_eqt  # noqa: F401
from . import spectrogram  # noqa: F401
from .spectrogram import Spectrogram, release_spectrogram_scratch  # noqa: F401
from . import trigger  # noqa: F401
from .trigger import (classic_sta_lta, recursive_sta_lta, release_trigger_scratch, sta_lta_triggers,  # noqa: F401
                      trigger_onset)

__version__ = "0.1.0"
