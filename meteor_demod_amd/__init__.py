"""meteor_demod_amd — MI355X-native LRPT demodulator (IQ in -> soft QPSK out).

Drop-in for the demod.c / dsp/ path of dbdexter-dev/meteor_demod behind a C-ABI
(include/meteor_demod_amd.h).  This package holds the HIP kernels (csrc/), the
built shared library (lib/) and a thin host-side mirror of the reference's
interface (demod.py).  Nothing here computes on the CPU.
"""
from .demod import DemodConfig, Demodulator, derive_tables, scale_freq_max  # noqa: F401
from .frontend import FrontEnd, FrontEndConfig, demodulate_recording_frontend, design_taps  # noqa: F401
from . import survey  # noqa: F401
from .survey import Hit, survey_plan  # noqa: F401
from . import frames  # noqa: F401
from .frames import Frame  # noqa: F401
from . import rs  # noqa: F401
from .rs import RsInfo  # noqa: F401
from . import interleave  # noqa: F401

__all__ = ["DemodConfig", "Demodulator", "derive_tables", "scale_freq_max",
           "FrontEnd", "FrontEndConfig", "demodulate_recording_frontend", "design_taps",
           "survey", "Hit", "survey_plan", "frames", "Frame", "rs", "RsInfo", "interleave"]
