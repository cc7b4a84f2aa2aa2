"""MI355X-native PSF reconstruction for MUSE WFM-AO (hot path of musevlt/muse-psfr).

Drop-in API (mirrors muse_psfr/psfrec.py of the reference): compute_psf, compute_psf_from_sparta,
create_sparta_table, fit_psf_cube, muse_intrinsic_psf, fit_psf_with_polynom, and the stages
simul_psd_wfm, psf_muse, convolve_final_psf,
psd_to_psf and its helpers pupil_mask, crop, interpolate, seeing2r01.
Beyond the reference: compute_field_psf (one PSF per field position) and the PSF_FIELD / FIT_FIELD HDUs of
compute_psf_from_sparta(..., field_positions=...); compute_profile_psf (a Cn2 profile of up to 8 layers with
per-layer wind, averaged or at field positions); compute_band_psf and band_weights (band-integrated PSFs of broadband
images) and the FIT_BAND_ROWS / PSF_BAND / FIT_BAND HDUs of compute_psf_from_sparta(..., bands=...).
psf_metrics (encircled / ensquared energy with exact pixel overlap and EE radii of any stamps), the metrics= argument
of the compute_* functions and the METRICS_* HDUs of compute_psf_from_sparta(..., metrics=...).
fit_stars_with_psf (PSF-fitting photometry: a model stamp, e.g. a reconstructed PSF, fitted to observed stars in flux,
sub-pixel shift and background) and fit_star_groups_with_psf (the same for blended stars: the two to four stars of a
stamp fitted at once); fit_star_spectra_with_psf (the spectrum of a star from its cube: one shared position, a flux
per wavelength).
cut_star_stamps, render_star_field and subtract_stars (the frame level of that photometry: stamps cut out of a frame,
model stars rendered into one, and the residual frame of a fit table -- all on the GPU) and find_stars (the stars of
a frame: matched-filter detection with the core of a model stamp, the source of the positions the others take);
group_stars (friends-of-friends groups of those stars: the blends that have to be fitted together, as the tables the
cut and the fits take) and fit_found_stars (group -> cut -> fit of the found stars, singles and blends, one table);
fit_crowded_stars (crowded-field photometry: the fluxes of all stars of a frame at known positions in one linear
solve, however many touch each other -- also the crowded='frame' mode of fit_found_stars), refine_crowded_stars (the
same with the positions free: fluxes and positions of all stars refined at once by Gauss-Newton -- also the
crowded='free' mode of fit_found_stars) and fit_crowded_spectra (the solve of fit_crowded_stars on every wavelength
layer of a cube, the layers side by side in one call: the spectra of all stars) and refine_crowded_spectra (the same
with ONE position per star refined from the layers jointly, every layer with its own PSF and refraction offset).
background_map (the sky of a frame or cube: a mesh of clipped medians, a smooth map of it and an rms map, all on the
GPU) and the sky= argument of fit_crowded_stars (fit, background of the residual, subtract, refit).
Low level: Context (ctypes binding of libmpsfr.so).
"""
from ._lib import Context, ContextPool, MpsfrError, NFIT, NFIT_ELL, NMET_HEAD, FIT_ILL_CONDITIONED, FIT_BACKGROUND, FIT_ELLIPTICAL, NFIT_PSF, FIT_FIXED_SHIFT, NFIT_GROUP, MAX_GROUP, FIT_COMMON_SHIFT, NFIT_SPEC, NFIT_SPEC_LAYER, FIT_DRIFT, NRENDER, RENDER_SUBTRACT, RENDER_SORT_CHUNK, NFIND, FIND_MAX_HALF, FIND_MAX_SEP, NGROUP, GROUP_MAX_CRIT, GROUP_OVERSIZE, GROUP_WIDE, NFRAMEFIT, FRAME_FIT_MAX_RADIUS, CUBE_FIT_MAX_LAYERS, NFRAMEFREE, NFRAMEFREE_HEAD, FRAME_FREE_MAX_OUTER, FRAME_FREE_MAX_STEP, FRAME_FREE_MAX_MOVE, FRAME_FREE_HELD, FRAME_FREE_BOUND, FRAME_FREE_CLIPPED, NCUBEFREE_POS, NCUBEFREE_CALL, CUBE_FREE_WORK_BYTES, NBACK, NBACK_HEAD, BACKGROUND_MIN_BOX, BACKGROUND_MAX_BOX, BACKGROUND_MAX_CLIP, BACK_FILLED, BACK_CLIP_CAP, BACK_FLAT  # noqa: F401
from .synthetic import synthetic_rows, grid_pixscale  # noqa: F401
from .psfrec import (MAX_L0, MIN_L0, compute_psf, compute_field_psf, compute_profile_psf,  # noqa: F401
                     band_weights, compute_band_psf, psf_metrics, fit_stars_with_psf, fit_star_groups_with_psf,
                     fit_star_spectra_with_psf, cut_star_stamps, render_star_field, subtract_stars, find_stars,
                     group_stars, fit_found_stars, fit_crowded_stars, refine_crowded_stars, fit_crowded_spectra,
                     refine_crowded_spectra, background_map,
                     compute_psf_from_sparta,
                     create_sparta_table, direction_perf, fit_psf_cube, fit_psf_with_polynom,
                     host_cutoff_masks, muse_intrinsic_psf, plot_psf, radial_profile,
                     simul_psd_wfm, psf_muse, convolve_final_psf, psd_to_psf, pupil_mask, crop,
                     interpolate, seeing2r01)

__version__ = '0.1.0'
