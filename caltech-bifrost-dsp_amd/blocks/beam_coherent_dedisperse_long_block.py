"""BeamCoherentDedisperseLong: BeamCoherentDedisperse for the sweeps that need transforms of 2^14 to 2^20 points.

BeamCoherentDedisperse filters every row inside one work-group's LDS, which ends at 2^13 points: with an overlap of 1.5 sweeps in
half a transform that shuts out the band below about 28 MHz at DM 10, below 37 MHz at the DM of B0329+54 and below 47 MHz at the
Crab's.  This block is that block -- ring formats, the header keys cdedisp_dm / cdedisp_nfft / cdedisp_overlap, the sequence, gap and
short-gulp rules, the `dms` command, the staging and stream declarations -- on a second engine, xengCdlong* (csrc/cdlong_kernels.h; the
definition is in include/xeng.h): a four-step FFT through a scratch buffer in device memory.  What is behind it (UpchanSumBeams,
BeamFold, BeamformVlbiOutput) reads its ring as it reads BeamCoherentDedisperse's.

It differs in three ways: the backend's cdlong_* methods; nfft from 2^14 to 2^20, planned by cdedisp_plan_long; and the chirp built
and uploaded pair by pair -- at 96 channels x 16 pairs and 2^17 points the whole table is 1.6 GB in complex64 and twice that in the
float64 it is rounded from, a pair's is a sixteenth of it."""
import numpy as np

from .beam_coherent_dedisperse_block import BeamCoherentDedisperse
from .coherent_dedisp import NFFT_LONG_MAX, NFFT_LONG_MIN, cdedisp_plan_long, chirp_table


class BeamCoherentDedisperseLong(BeamCoherentDedisperse):
    WHO = "BEAM_COHERENT_DEDISPERSE_LONG"
    ENGINE = 'cdlong'
    RUN_NAME = "xengCdlongRun"
    NFFT_RANGE = (NFFT_LONG_MIN, NFFT_LONG_MAX, "2^14 to 2^20")
    plan = staticmethod(cdedisp_plan_long)

    def _upload_chirp(self, freqs, chan_bw):
        for p, dm in enumerate(self.dms):
            self._call('cdlong_set_chirp', p, np.ascontiguousarray(chirp_table(freqs, chan_bw, [dm], self.nfft)[0]))
