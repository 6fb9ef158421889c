"""Hot-path blocks with the reference's Block + ring interface."""
from .block_base import Block, COMMAND_OK, COMMAND_NOT_RECOGNIZED, COMMAND_WRONG_TYPE, COMMAND_INVALID
from .corr_block import Corr, regtile_index, tri_index
from .corr_acc_block import CorrAcc
from .beamform_block import Beamform
from .beamform_sum_beams_block import BeamformSumBeams
from .copy_block import Copy
from .corr_subsel_block import CorrSubsel
from .corr_output_full_block import CorrOutputFull
from .snap2_ingest_block import Snap2Ingest
from .beamform_output_block import BeamformOutput
from .corr_output_part_block import CorrOutputPart
from .beamform_vlbi_output_block import BeamformVlbiOutput
from .upchan_beamform_block import UpchanBeamform
from .tbf_source_block import TbfSource
from .upchan_corr_block import UpchanCorr
from .upchan_sum_beams_block import UpchanSumBeams
from .upchan_spectra_block import UpchanSpectra
from .beam_dedisperse_block import BeamDedisperse
from .dedisp import dm_delays
from .beam_pulse_search_block import BeamPulseSearch
from .pulse_search import pulse_candidates
from .beam_period_search_block import BeamPeriodSearch
from .period_search import period_candidates, period_pfa
from .beam_period_search_long_block import BeamPeriodSearchLong
from .period_search import period_bands, period_candidates_long, period_sift
from .beam_accel_search_block import BeamAccelSearch
from .accel_search import ACCEL_RECORD, accel_alpha, accel_candidates, accel_index, accel_of, accel_trials, as_records_accel
from .beam_ffa_search_block import BeamFfaSearch
from .ffa_search import ffa_candidates, ffa_period, ffa_plan, ffa_rows
from .beam_cand_fold_block import BeamCandFold
from .cand_fold import (CANDFOLD_RECORD, as_records_candfold, candfold_candidates, candfold_gains, candfold_oscillators, candfold_refined, candfold_shifts,
                        candfold_sigma, candfold_trials)
from .beam_rfi_clean_block import BeamRfiClean
from .rfi_clean import rfi_controls, rfi_mad, rfi_median, rfi_occupancy, rfi_tree_sum, rfi_weights
from .beam_detrend_block import BeamDetrend
from .detrend import detrend_k_mad, detrend_plan, detrend_reference, detrend_startup
from .beam_pulse_cutout_block import BeamPulseCutout
from .pulse_cutout import (CUTOUT_RECORD, CUTOUT_REQUEST, CutoutQueue, as_cutouts, cutout_fine_dms, cutout_k_mad, cutout_offsets, cutout_plan, cutout_reference,
                           cutout_refined, cutout_requests)
from .beam_rm_synth_block import BeamRmSynth
from .rm_synth import (RM_RECORD, as_rmsynth, pol_profile, rm_error, rm_lambda2, rm_offsets, rm_plan, rm_reference, rm_refine, rm_significance, rm_table,
                       rmsf)
from .beam_toa_block import BeamToa
from .toa import (TOA_RECORD, as_toa, subband_frequencies, toa_dm_fit, toa_epoch, toa_offsets, toa_reference, toa_refine, toa_subbands, toa_tables,
                  toa_template)
from .beam_fold_block import BeamFold
from .fold import fold_phase, fold_rotations, fold_rotations_coherent, profile_snr
from .beam_coherent_dedisperse_block import BeamCoherentDedisperse
from .beam_coherent_dedisperse_long_block import BeamCoherentDedisperseLong
from .coherent_dedisp import cdedisp_plan, cdedisp_plan_long, chirp_table, smear_samples
from .upchan_image_block import UpchanImage
from .upchan_clean_block import UpchanClean
from .imaging import (clean_components, clean_layout, component_visibilities, components_to_model, direction_list, image_norm, patch, pixel_grid, psf, restore,
                      steering_delays, stokes_i)
from .upchan_gaincal_block import UpchanGainCal
from .upchan_calapply_block import UpchanCalApply
from .upchan_peel_block import UpchanPeel
from .upchan_flag_block import UpchanFlag
from .upchan_predict_block import UpchanPredict
from .upchan_image_search_block import UpchanImageSearch
from .image_search import IMSEARCH_RECORD, group_frequencies, image_candidates, image_dm_delays
from .flagging import flag_factors, flag_summary, flag_visibilities, stand_weights
from .calibration import apply_gains, direction_model_visibilities, inverse_gains, model_flux, model_visibilities, reference_phase
from .spectral_kurtosis import incoherent_beam, sk_flags, sk_limits, spectral_kurtosis

__all__ = ["Block", "Corr", "CorrAcc", "Beamform", "BeamformSumBeams", "Copy", "CorrSubsel", "CorrOutputFull", "Snap2Ingest", "BeamformOutput", "CorrOutputPart", "BeamformVlbiOutput", "UpchanBeamform", "TbfSource", "UpchanCorr", "UpchanSumBeams", "UpchanSpectra", "BeamDedisperse", "dm_delays", "BeamPulseSearch", "pulse_candidates", "BeamPeriodSearch", "BeamPeriodSearchLong", "period_bands", "period_candidates_long", "period_sift", "BeamAccelSearch", "ACCEL_RECORD", "accel_alpha", "accel_of", "accel_index", "accel_trials", "accel_candidates", "as_records_accel", "BeamFfaSearch", "period_candidates", "period_pfa", "ffa_candidates", "ffa_period", "ffa_plan", "ffa_rows", "BeamCandFold", "CANDFOLD_RECORD", "as_records_candfold", "candfold_candidates", "candfold_gains", "candfold_oscillators", "candfold_refined", "candfold_shifts", "candfold_sigma", "candfold_trials", "BeamRfiClean", "rfi_controls", "rfi_mad", "rfi_median", "rfi_occupancy", "rfi_tree_sum", "rfi_weights", "BeamDetrend", "detrend_k_mad", "detrend_plan", "detrend_reference", "detrend_startup", "BeamPulseCutout", "CUTOUT_RECORD", "CUTOUT_REQUEST", "CutoutQueue", "as_cutouts", "cutout_fine_dms", "cutout_k_mad", "cutout_offsets", "cutout_plan", "cutout_reference", "cutout_refined", "cutout_requests", "BeamRmSynth", "RM_RECORD", "as_rmsynth", "pol_profile", "rm_error", "rm_lambda2", "rm_offsets", "rm_plan", "rm_reference", "rm_refine", "rm_significance", "rm_table", "rmsf", "BeamToa", "TOA_RECORD", "as_toa", "subband_frequencies", "toa_dm_fit", "toa_epoch", "toa_offsets", "toa_reference", "toa_refine", "toa_subbands", "toa_tables", "toa_template", "BeamFold", "fold_phase", "fold_rotations", "fold_rotations_coherent", "profile_snr", "BeamCoherentDedisperse", "BeamCoherentDedisperseLong", "chirp_table", "smear_samples", "cdedisp_plan", "cdedisp_plan_long", "UpchanImage", "pixel_grid", "patch", "steering_delays", "direction_list", "image_norm", "stokes_i", "UpchanClean", "psf", "clean_components", "clean_layout", "restore", "components_to_model", "UpchanGainCal", "UpchanCalApply", "UpchanPeel", "UpchanFlag", "UpchanPredict", "component_visibilities", "UpchanImageSearch", "IMSEARCH_RECORD", "group_frequencies", "image_dm_delays", "image_candidates", "flag_factors", "stand_weights", "flag_visibilities", "flag_summary", "model_visibilities", "direction_model_visibilities", "model_flux", "apply_gains", "inverse_gains", "reference_phase", "spectral_kurtosis", "sk_limits", "sk_flags", "incoherent_beam", "regtile_index", "tri_index",
           "COMMAND_OK", "COMMAND_NOT_RECOGNIZED", "COMMAND_WRONG_TYPE", "COMMAND_INVALID"]
