/*
 * clsimhip.h -- C ABI of the MI355X photon propagator (libclsimhip.so).
 *
 * This is the drop-in boundary behind clsim's step->photon converter: every
 * entry point replaces one member of the reference's C++ interface
 *   public/clsim/I3CLSimStepToPhotonConverter.h:67-192        (abstract interface)
 *   public/clsim/I3CLSimStepToPhotonConverterOpenCL.h:78-258  (concrete setters)
 * or one host helper the canonical caller uses to configure it
 *   private/clsim/I3CLSimModuleHelper.cxx:175-372, python/MakeIceCubeMediumProperties.py,
 *   python/GetIceCubeDOMAcceptance.py, private/opencl/mwcrng_init.h.
 * Plain pointers and sizes only; no C++ / torch types.  All functions return
 * CLSIMHIP_OK (0) or a negative status; clsimhip_last_error() gives the text
 * (the reference throws I3CLSimStepToPhotonConverter_exception with that text).
 *
 * Records are the reference's packed little-endian wire structs:
 *   step   48 B  public/clsim/I3CLSimStep.h:141-155
 *   photon 80 B  public/clsim/I3CLSimPhoton.h:194-213
 */
#ifndef CLSIMHIP_H
#define CLSIMHIP_H

#ifndef __HIPCC_RTC__      /* (the device headers include this file for its constants; the run-time compiler has no C library) */
#include <stddef.h>
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define CLSIMHIP_OK 0
#define CLSIMHIP_ERR_ARGUMENT (-1)  /* null / empty / out-of-range argument            */
#define CLSIMHIP_ERR_STATE (-2)     /* setter after Initialize, use before Initialize   */
#define CLSIMHIP_ERR_CONFIG (-3)    /* configuration this build cannot run              */
#define CLSIMHIP_ERR_DEVICE (-4)    /* HIP runtime error / no GPU                       */
#define CLSIMHIP_ERR_IO (-5)        /* file not found / malformed table                 */

typedef struct clsimhip_converter clsimhip_converter;
typedef struct clsimhip_medium clsimhip_medium;

/* I3CLSimStep (48 B) and I3CLSimPhoton (80 B), byte-compatible with the reference. */
#pragma pack(push, 1)
typedef struct {
    float x, y, z, time;
    float theta, phi, length, beta;
    uint32_t num_photons;
    float weight;
    uint32_t identifier;
    uint8_t source_type, dummy1;
    uint16_t dummy2;
} clsimhip_step;
typedef struct {
    float x, y, z, time;
    float theta, phi, wavelength, cherenkov_dist;
    uint32_t num_scatters;
    float weight;
    uint32_t identifier;
    int16_t string_id;
    uint16_t om_id;
    float start_x, start_y, start_z, start_time;
    float start_theta, start_phi, group_velocity, dist_in_abs_lens;
} clsimhip_photon;
#pragma pack(pop)

/* ---- value descriptions (doubles, like the reference's function objects) ---- */

/* I3CLSimFunction: FromTable (equal spacing) or Constant.
 * private/clsim/function/I3CLSimFunctionFromTable.cxx:70-90, ...Constant.cxx:40-44.
 * Two more kinds exist on the host only, as the emission spectra handed to clsimhip_make_wlen_generator -- like the reference,
 * whose FromTable has no device code for unequal spacing (FromTable.cxx:169-170) and whose DeltaPeak is turned into a constant
 * generator (I3CLSimModuleHelper.cxx:78-89): a converter refuses them as wavelength bias, a medium as refractive index. */
#define CLSIMHIP_FUNCTION_TABLE 0
#define CLSIMHIP_FUNCTION_CONSTANT 1
#define CLSIMHIP_FUNCTION_TABLE_X 2     /* FromTable(wlens, values), FromTable.cxx:57-70: n wavelengths (ascending) + n values */
#define CLSIMHIP_FUNCTION_DELTA_PEAK 3  /* I3CLSimFunctionDeltaPeak: value = the peak's wavelength */
typedef struct {
    int32_t kind;
    int32_t n;               /* TABLE, TABLE_X: number of entries (>=2)   */
    double start, step;      /* TABLE: first wavelength, spacing [m]      */
    const double *values;    /* TABLE, TABLE_X: n values                  */
    double value;            /* CONSTANT; DELTA_PEAK: peak position [m]   */
    const double *wavelengths; /* TABLE_X: n wavelengths [m]              */
} clsimhip_function;

/* I3CLSimRandomValue used as wavelength generator: InterpolatedDistribution
 * (constant x spacing, or with its own x values: the flasher LEDs' measured spectra) or Constant (delta peak).
 * private/clsim/random_value/I3CLSimRandomValueInterpolatedDistribution.cxx:40-74 */
#define CLSIMHIP_RANDOM_INTERPOLATED 0
#define CLSIMHIP_RANDOM_CONSTANT 1
#define CLSIMHIP_RANDOM_CHERENKOV_NO_DISPERSION 2 /* I3CLSimRandomValueWlenCherenkovNoDispersion(fromWlen, toWlen)
                                                    (random_value/…WlenCherenkovNoDispersion.cxx:40-98): first = fromWlen,
                                                    spacing = toWlen */
#define CLSIMHIP_RANDOM_INTERPOLATED_X 3 /* InterpolatedDistribution(x, y), InterpolatedDistribution.cxx:40-55 */
typedef struct {
    int32_t kind;
    int32_t n;
    double first, spacing;   /* INTERPOLATED: x of first point, x spacing  */
    const double *y;         /* INTERPOLATED, INTERPOLATED_X: n unnormalised densities */
    double value;            /* CONSTANT                                    */
    const double *x;         /* INTERPOLATED_X: n abscissae, ascending      */
} clsimhip_random_value;

/* I3CLSimMediumProperties restricted to the function classes of the IceCube
 * ice models (public/clsim/I3CLSimMediumProperties.h:54-200). */
#define CLSIMHIP_LENGTHS_CONSTANT 0 /* I3CLSimFunctionConstant per layer          */
#define CLSIMHIP_LENGTHS_ICECUBE 1  /* I3CLSimFunctionAbsLenIceCube/ScatLenIceCube */
#define CLSIMHIP_LENGTHS_TABLE 2    /* one I3CLSimFunctionFromTable per layer (photonics ice tables) */
#define CLSIMHIP_REFINDEX_ICECUBE 0 /* I3CLSimFunctionRefIndexIceCube (n[] / g[])  */
#define CLSIMHIP_REFINDEX_TABLE 1   /* I3CLSimFunctionFromTable, same function for every layer */
#define CLSIMHIP_REFINDEX_DISPERSION 2 /* group_index_kind only: NO group refractive index override is set; the group velocity comes from the
                                        * phase index and its derivative (I3CLSimHelperGenerateMediumPropertiesSource.cxx:274-300,
                                        * I3CLSimFunctionRefIndexIceCube.cxx:205-215).  Needs phase_index_kind ICECUBE: FromTable has no
                                        * derivative (I3CLSimFunctionFromTable.h:67).  The table maker refuses it as the reference does
                                        * (I3CLSimStepToTableConverter.cxx:103-104) */
#define CLSIMHIP_SCATTER_HG 0
#define CLSIMHIP_SCATTER_LIU 1
#define CLSIMHIP_SCATTER_MIXED 2    /* Mixed(SimplifiedLiu, HenyeyGreenstein, f)   */
typedef struct {
    int32_t num_layers;
    double layers_z_start, layers_height;
    double min_wavelength, max_wavelength;          /* ForcedMinWlen / ForcedMaxWlen */
    int32_t lengths_kind;
    const double *abs_length, *sca_length;          /* CONSTANT: per layer [m]        */
    double alpha, kappa, A, B, D, E;                /* ICECUBE                         */
    const double *a_dust400, *delta_tau, *b400;     /* ICECUBE: per layer, bottom->top */
    double n[5], g[5];                              /* RefIndexIceCube phase / group   */
    int32_t scatter_kind;
    double liu_fraction, mean_cosine;
    int32_t has_anisotropy;                         /* ScalarFieldAnisotropyAbsLenScaling */
    double aniso_azimuth, aniso_k1, aniso_k2;
    int32_t has_pre_transform, pre_renormalize;     /* VectorTransformMatrix            */
    double pre_matrix[9];
    int32_t has_post_transform, post_renormalize;
    double post_matrix[9];
    int32_t has_tilt;                               /* ScalarFieldIceTiltZShift          */
    int32_t tilt_num_distances, tilt_num_z;
    const double *tilt_distances, *tilt_z_coordinates, *tilt_z_corrections; /* [nd][nz] */
    double tilt_azimuth;
    /* TABLE lengths (private/clsim/function/I3CLSimFunctionFromTable.cxx:167-300): equal spacing common to
     * all layers; store_as_16bit = storeDataAsHalfPrecision (linear 16-bit quantisation between the
     * smallest and largest entry of each function) */
    int32_t table_num_wavelengths;
    double table_start_wavelength, table_wavelength_step;
    int32_t table_store_as_16bit;
    const double *abs_length_table, *sca_length_table; /* [num_layers][table_num_wavelengths], metres */
    /* refractive indices; the propagator needs a layer independent group velocity
     * (propagation_kernel.c.cl:525-527), so there is one function of each kind */
    int32_t phase_index_kind, group_index_kind;         /* CLSIMHIP_REFINDEX_* */
    clsimhip_function phase_index_table, group_index_table; /* kind TABLE */
} clsimhip_medium_desc;

/* ---- medium objects ---- */
/* deep copy of a description */
int clsimhip_medium_create(const clsimhip_medium_desc *desc, clsimhip_medium **out);
/* python/MakeIceCubeMediumProperties.py:49-256: PPC ice tables (icemodel.dat/.par,
 * cfg.txt[, tilt.dat/.par]) -> medium */
int clsimhip_medium_create_from_ppc(const char *directory, double detector_center_depth,
                                    int use_tilt_if_available, clsimhip_medium **out);
/* python/MakeIceCubeMediumPropertiesPhotonics.py:47-227: photonics ice table file (NLAYER / NWVL / per layer
 * LAYER, ABS, SCAT, COS, N_GROUP, N_PHASE) -> medium with tabulated lengths and refractive indices */
int clsimhip_medium_create_from_photonics(const char *table_file, double detector_center_depth, clsimhip_medium **out);
/* view into the object's own arrays (valid until destroy) */
int clsimhip_medium_describe(const clsimhip_medium *m, clsimhip_medium_desc *out);
void clsimhip_medium_destroy(clsimhip_medium *m);

/* python/GetIceCubeDOMAcceptance.py:35-115 (43 entries, 260..680 nm); values_out[43] */
int clsimhip_icecube_dom_acceptance(double dom_radius, double efficiency, double *values_out,
                                    double *start_out, double *step_out);
/* I3CLSimModuleHelper::makeCherenkovWavelengthGenerator, tabulated bias
 * (I3CLSimModuleHelper.cxx:175-263): y_out[bias->n] */
int clsimhip_make_cherenkov_wlen_generator(const clsimhip_function *bias, const clsimhip_medium *m,
                                           double *y_out, double *first_out, double *spacing_out);

/* I3CLSimModuleHelper::makeWavelengthGenerator (I3CLSimModuleHelper.cxx:73-171) for the spectrum classes its callers pass
 * (python/GetIceCubeFlasherSpectrum.py): DELTA_PEAK -> CONSTANT; TABLE / TABLE_X -> INTERPOLATED / INTERPOLATED_X on the
 * table's own binning, every entry multiplied by the bias at its wavelength.  `out` is filled in with out->y = y_out and
 * out->x = x_out (x_out only written for INTERPOLATED_X); both arrays hold `capacity` >= spectrum->n doubles. */
int clsimhip_make_wlen_generator(const clsimhip_function *spectrum, const clsimhip_function *bias, const clsimhip_medium *m,
                                 clsimhip_random_value *out, double *x_out, double *y_out, size_t capacity);

/* ---- RNG set-up (private/opencl/mwcrng_init.h:26-117, private/make_safeprimes/main.cxx) ---- */
/* first `count` MWC multipliers (a*2^32-1 and (a*2^32-2)/2 prime, descending from 4294967118) */
int clsimhip_mwc_multipliers(uint32_t *a_out, size_t count);
/* first `count` multipliers from a safeprimes file in one of the reference's formats (mwcrng_init.h:62-103:
 * 17-byte tag "safeprimes_base32" + little-endian int64 each, or text with the multiplier in column 1) */
int clsimhip_mwc_multipliers_from_file(const char *path, uint32_t *a_out, size_t count);
/* state words with init_MWC_RNG's validity loop; draws come from splitmix64(seed) */
int clsimhip_seed_streams(const uint32_t *a, size_t count, uint64_t seed, uint64_t *x_out);

/* ---- converter life cycle (I3CLSimStepToPhotonConverterOpenCL.cxx:68-388) ---- */
int clsimhip_create(int device_ordinal, clsimhip_converter **out);
void clsimhip_destroy(clsimhip_converter *c);
/* Text of the last failure of a clsimhip_* call made BY THE CALLING THREAD (thread-local, like errno; `c` is ignored and
 * may be NULL): the interface is driven by several threads per converter (I3CLSimServer.cxx:126-135, 324-331). */
const char *clsimhip_last_error(const clsimhip_converter *c);
/* SetDevice (public/clsim/I3CLSimStepToPhotonConverterOpenCL.h:96-103, OpenCL.cxx:1322-1331; the canonical caller's
 * first call, I3CLSimModuleHelper.cxx:321): the HIP device ordinal replaces the I3CLSimOpenCLDevice.  Before Initialize. */
int clsimhip_set_device(clsimhip_converter *c, int device_ordinal);
int clsimhip_get_device(const clsimhip_converter *c, int *out);
/* Device errors: a HIP error inside the converter's worker thread is where the reference log_fatal()s and exits
 * (OpenCL.cxx:768-774).  This library does not end its host: the worker stops, blocked callers wake up, and every
 * later EnqueueSteps / GetConversionResult returns CLSIMHIP_ERR_DEVICE with the original text. */

/* setters: CLSIMHIP_ERR_STATE once initialized (OpenCL.cxx:1322-1523) */
int clsimhip_set_wlen_generators(clsimhip_converter *c, const clsimhip_random_value *gens, size_t n);
int clsimhip_set_wlen_bias(clsimhip_converter *c, const clsimhip_function *bias);
int clsimhip_set_medium_properties(clsimhip_converter *c, const clsimhip_medium *m);
/* I3CLSimSimpleGeometry: parallel arrays, one entry per DOM (public/clsim/I3CLSimSimpleGeometry.h) */
int clsimhip_set_geometry(clsimhip_converter *c, size_t n, const int32_t *string_ids, const uint32_t *dom_ids,
                          const double *x, const double *y, const double *z,
                          const char *const *subdetectors, double om_radius);
/* I3CLSimSimpleGeometryTextFile (private/clsim/I3CLSimSimpleGeometryTextFile.cxx:43-100): whitespace separated
 * "string dom x y z" records; strings / DOMs outside [*_min, *_max] are ignored (reference defaults: 1..INT32_MAX,
 * 1..60); every DOM is in the subdetector "default" */
int clsimhip_set_geometry_from_text_file(clsimhip_converter *c, const char *filename, double om_radius,
                                         int32_t string_id_min, int32_t string_id_max, uint32_t dom_id_min, uint32_t dom_id_max);
int clsimhip_set_enable_double_buffering(clsimhip_converter *c, int value);
int clsimhip_set_double_precision(clsimhip_converter *c, int value);           /* only 0 */
int clsimhip_set_stop_detected_photons(clsimhip_converter *c, int value);      /* 0 (the default, as in the reference class, OpenCL.cxx:86; initializeOpenCL's callers pass 1): every DOM on a photon's way records it and the photon travels on (no STOP_PHOTONS_ON_DETECTION) */
int clsimhip_set_save_all_photons(clsimhip_converter *c, int value);           /* only 0 */
int clsimhip_set_save_all_photons_prescale(clsimhip_converter *c, double value);
int clsimhip_set_fixed_number_of_absorption_lengths(clsimhip_converter *c, double value); /* NaN = off */
int clsimhip_set_dom_pancake_factor(clsimhip_converter *c, double value);
int clsimhip_set_photon_history_entries(clsimhip_converter *c, uint32_t value); /* only 0 */
int clsimhip_set_workgroup_size(clsimhip_converter *c, size_t value);
int clsimhip_set_max_num_workitems(clsimhip_converter *c, size_t value);
/* Compile(): build the device tables from the configuration (OpenCL.cxx:485-533) */
int clsimhip_compile(clsimhip_converter *c);
int clsimhip_get_max_workgroup_size(const clsimhip_converter *c, size_t *out);
/* Initialize(): RNG streams a[i] = i-th multiplier, x[i] seeded from `seed` (OpenCL.cxx:217-388) */
int clsimhip_initialize(clsimhip_converter *c, uint64_t seed);
/* same with caller-supplied streams (count must equal max_num_workitems) */
int clsimhip_initialize_with_streams(clsimhip_converter *c, const uint64_t *x, const uint32_t *a, size_t count);
int clsimhip_is_initialized(const clsimhip_converter *c);

/* ---- steady state (OpenCL.cxx:1525-1640) ---- */
/* EnqueueSteps: copies `n` steps; blocks while 5 bunches are pending.  n must be
 * non-zero, <= max_num_workitems and a multiple of the workgroup size. */
int clsimhip_enqueue_steps(clsimhip_converter *c, const clsimhip_step *steps, size_t n, uint32_t identifier);
/* GetConversionResult: blocks for the next finished bunch.  String/DOM indices are
 * already replaced by IDs.  *photons stays valid until clsimhip_release_result. */
int clsimhip_get_conversion_result(clsimhip_converter *c, uint32_t *identifier,
                                   const clsimhip_photon **photons, size_t *n);
/* ConversionResult_t::photonHistories (I3CLSimStepToPhotonConverter.h:70-90) of the result that `photons` belongs to,
 * as ConvertPhotonHistories builds them (OpenCL.cxx:940-989): `*entries` float[4] records per photon {x, y, z,
 * absorption lengths travelled} in forward order (most recent scatter last); photon i has
 * min(numScatters_i, *entries) of them, the rest of its block is zero.  *histories is NULL when
 * PhotonHistoryEntries is 0 or the result is empty; valid until clsimhip_release_result(photons). */
int clsimhip_get_result_histories(clsimhip_converter *c, const clsimhip_photon *photons, const float **histories,
                                  uint32_t *entries);
int clsimhip_release_result(clsimhip_converter *c, const clsimhip_photon *photons);
int clsimhip_get_workgroup_size(const clsimhip_converter *c, size_t *out);
int clsimhip_get_max_num_workitems(const clsimhip_converter *c, size_t *out);
int clsimhip_queue_size(const clsimhip_converter *c, size_t *out);
int clsimhip_more_photons_available(const clsimhip_converter *c, int *out);
/* GetStatistics(): [0] TotalDeviceTime ns, [1] TotalHostTime ns, [2] NumKernelCalls,
 * [3] TotalNumPhotonsGenerated, [4] TotalNumPhotonsAtDOMs, [5] AverageDeviceTimePerPhoton,
 * [6] AverageHostTimePerPhoton, [7] DeviceUtilization */
int clsimhip_get_statistics(const clsimhip_converter *c, double out[8]);
/* the option getters of the concrete class (GetEnableDoubleBuffering ... GetDOMPancakeFactor, OpenCL.h:138-258): what the
 * setters stored */
#define CLSIMHIP_OPTION_ENABLE_DOUBLE_BUFFERING 0
#define CLSIMHIP_OPTION_DOUBLE_PRECISION 1
#define CLSIMHIP_OPTION_STOP_DETECTED_PHOTONS 2
#define CLSIMHIP_OPTION_SAVE_ALL_PHOTONS 3
#define CLSIMHIP_OPTION_SAVE_ALL_PHOTONS_PRESCALE 4
#define CLSIMHIP_OPTION_FIXED_NUMBER_OF_ABSORPTION_LENGTHS 5    /* NaN: not set */
#define CLSIMHIP_OPTION_DOM_PANCAKE_FACTOR 6
#define CLSIMHIP_OPTION_PHOTON_HISTORY_ENTRIES 7
int clsimhip_get_option(const clsimhip_converter *c, int option, double *out);

/* ---- tuning (no reference counterpart; the reference's one launch parameter is the work-group size it takes from
 * the device, OpenCL.cxx:520-560) ----
 * The launcher's parameters have defaults found by measurement; a caller who knows its bunches better
 * sets them here.  NO RESULT DEPENDS ON ANY OF THEM: every schedule gives the same photon records and the same final
 * RNG states (tests/test_stress_schedules_gpu.py).  The library reads NO tuning from the environment (a build with
 * -DCLSIMHIP_DEVELOPER, `make DEVELOPER=1`, honours the round 1-5 variable names for the measurement tools under
 * tools/); the only environment variables of the default build are CLSIMHIP_SAFEPRIMES_FILE (a file of multipliers
 * in the reference's format, mwcrng_init.h:44-82) and CLSIMHIP_RCCL_LIBRARY (which RCCL to dlopen).
 *
 *   key                  values           meaning (default)
 *   "kernel"             0 | 1 | 2        0: pooled kernel for bunches of at least "pool_min_steps" steps, classic below; 1: pooled,
 *                                         2: classic, for every bunch size (0)
 *   "pool_min_steps"     -1 | >= 0        smallest bunch the pooled kernel takes; -1: 524 288, or 0 when "kernel" is 1 (-1)
 *   "pool_max_steps"     -1 | >= 1        largest bunch the pooled kernel takes; can only lower the limit of its 23-bit step index (-1)
 *   "pool_ring"          0 ... 4096       pooled kernel: created photons a wave keeps ready; 0: what the LDS holds, 45 for IceCube (0)
 *   "k_new"              0 ... 4096       lanes / ring entries waiting before a wave creates photons; 0: automatic (0)
 *   "k_search"           0 ... 64         lanes parked before a wave searches for DOMs; 0: automatic (0)
 *   "slices"             0 ... 65535      work units a step is cut into; 0: 16, or 1 for bunches smaller than the grid (0)
 *   "k_pop"              0 ... 64         pooled kernel: free lanes before a wave hands out ready photons; 0: 4 (0)
 *   "k_wait"             -1 ... 255       pooled kernel: trips a parked lane waits for company; -1: 16; 0: never (-1)
 *   "k_aim"              -1 ... 64        pooled kernel: lanes at a string up to which the "aimed at the string?" level is asked;
 *                                         -1: 8; 0: the level is off (-1)
 *   "grid"               0 ... 2^20       workgroups of the propagation launch; 0: what the chip holds, cut to the work (0)
 *   "generic_kernels"    0 | 1            1: the generic instantiation also where Compile() found every proof of the fast one (0)
 *   "result_min_records" >= 1             smallest page-locked result buffer, in photon records (65 536)
 *   -- the three below shape tables of Compile(): CLSIMHIP_ERR_STATE after Compile() --
 *   "string_map_cells"   8 ... 4096       string proximity map, cells per axis (512)
 *   "dom_map_cells"      4 ... 512        DOM proximity map, largest number of cubic cells per axis (256)
 *   "named_search"       0 | 1            0: every DOM takes the full search instead of the one confined to the named DOM (1)
 * Any other key or value: CLSIMHIP_ERR_ARGUMENT.  May be called between bunches at any time; a launch reads the values
 * when it is queued. */
int clsimhip_set_tuning(clsimhip_converter *c, const char *key, long long value);
int clsimhip_get_tuning(const clsimhip_converter *c, const char *key, long long *value);

/* ---- device-resident path (no reference counterpart: the reference always
 * stages through host memory, OpenCL.cxx:824-911, 994-1086) ----
 * Propagates n steps that already live in HBM, on the caller's HIP stream
 * (hipStream_t passed as void*; NULL = default stream).  d_photons has room for
 * `capacity` records, *d_hit_count (uint32, zeroed by this call) receives the
 * number of detected photons (may exceed capacity; only the first `capacity`
 * are stored).  rng_offset selects the first RNG stream used (stream i of the
 * bunch = rng_offset + i).  String/DOM fields hold INDICES.  Asynchronous. */
int clsimhip_propagate_device(clsimhip_converter *c, const void *d_steps, size_t n, size_t rng_offset,
                              void *d_photons, size_t capacity, void *d_hit_count, void *stream);
/* Small bunches: a launch is a persistent grid sized for the whole chip, and a bunch of a few 10^5 steps leaves most lanes
 * with less than one step.  A caller that has several such bunches keeps k of them in flight instead -- k calls of
 * clsimhip_propagate_device on k different HIP streams, over disjoint RNG stream ranges [rng_offset, rng_offset + n) and
 * with output buffers of their own -- after telling the converter so: every launch then sizes its grid for 1/k of the
 * chip and they run side by side (work records and queue heads are per stream range and per launch).  Results do not
 * depend on k.  1 <= k <= 16, default 1; may be changed between launches. */
int clsimhip_set_concurrent_device_launches(clsimhip_converter *c, int k);
/* index -> ID translation on the device records' host copy (OpenCL.cxx:1565-1600) */
int clsimhip_replace_indices_with_ids(const clsimhip_converter *c, clsimhip_photon *photons, size_t n);
/* average duration (ms) of the propagation kernel over the launches recorded since
 * the last call with reset!=0, measured with HIP events on the launch stream */
int clsimhip_kernel_time_ms(clsimhip_converter *c, int reset, double *total_ms, uint64_t *launches);

/* ---- wire format of step and photon series ------------------------------------------------
 * Payload of I3Vector<I3CLSimStep>::serialize / I3Vector<I3CLSimPhoton>::serialize for the portable binary archive
 * (private/clsim/I3CLSimStep.cxx:111-147, private/clsim/I3CLSimPhoton.cxx:141-168), the messages of I3CLSimServer /
 * I3CLSimClient (I3CLSimServer.cxx:320, 339, 386, 408): class version (0), number of records, then the records as one
 * little-endian blob -- from the class version on.  The archive framing around it (stream header, object tracking
 * records of the shared_ptr and of the I3FrameObject base) belongs to icecube::serialization, which is not part of the
 * reference tree; integers use that archive's published encoding (count byte + little-endian bytes). */
int clsimhip_step_series_blob_size(size_t n, size_t *bytes);
int clsimhip_encode_step_series(const clsimhip_step *steps, size_t n, uint8_t *out, size_t capacity, size_t *written);
/* *n = number of steps in the blob; steps_out may be NULL to ask for the count; *consumed (may be NULL) = bytes read */
int clsimhip_decode_step_series(const uint8_t *blob, size_t bytes, clsimhip_step *steps_out, size_t capacity, size_t *n, size_t *consumed);
int clsimhip_photon_series_blob_size(size_t n, size_t *bytes);
int clsimhip_encode_photon_series(const clsimhip_photon *photons, size_t n, uint8_t *out, size_t capacity, size_t *written);
int clsimhip_decode_photon_series(const uint8_t *blob, size_t bytes, clsimhip_photon *photons_out, size_t capacity, size_t *n, size_t *consumed);
/* the archive's unsigned integer encoding itself (out: up to 9 bytes) */
int clsimhip_encode_portable_uint(uint64_t value, uint8_t out[9], size_t *written);

/* ---- multi-GPU: gather of detected photons over RCCL / xGMI (no reference counterpart, the reference
 * collects the results of its per-device converters with host threads, I3CLSimServer.cxx:77-137) ----
 * One process (or thread) per GPU: each propagates a contiguous shard of the steps with clsimhip_propagate_device and
 * its own streams -- no exchange -- then the ranks' photons are gathered on `root`, rank by rank.  RCCL is loaded at
 * run time (dlopen; CLSIMHIP_RCCL_LIBRARY overrides the name): no link-time dependency. */
#define CLSIMHIP_UNIQUE_ID_BYTES 128
typedef struct clsimhip_comm clsimhip_comm;
/* ncclGetUniqueId: called by one rank; the host application hands the bytes to the others (MPI, ZMQ, a file ...) */
int clsimhip_comm_get_unique_id(uint8_t id[CLSIMHIP_UNIQUE_ID_BYTES]);
/* ncclCommInitRank on HIP device `device_ordinal`; collective: every rank of the job calls it */
int clsimhip_comm_create(int device_ordinal, int rank, int world_size, const uint8_t id[CLSIMHIP_UNIQUE_ID_BYTES], clsimhip_comm **out);
void clsimhip_comm_destroy(clsimhip_comm *comm);
/* What the communicator says about itself: ncclCommCount / ncclCommUserRank asked of the communicator after
 * ncclCommInitRank (clsimhip_comm_create fails when they differ from what the caller passed), the HIP device it lives on
 * and that device's PCI bus id (hipDeviceGetPCIBusId; "" if unknown).  A multi-GPU record quotes THESE numbers: N ranks
 * with N distinct bus ids.  The reference reports per-device statistics from its server (I3CLSimServer.cxx:355-368).
 * Any out pointer may be NULL. */
int clsimhip_comm_info(clsimhip_comm *comm, int *rccl_ranks, int *rccl_rank, int *device_ordinal, char *pci_bus_id, size_t pci_bus_id_bytes);
/* Gathers issued since creation (or the last reset): their number, the time they held the stream (HIP events around
 * each clsimhip_gather_hits on its stream; the call waits for the gathers issued so far), the photon records this rank
 * sent to a root / received as a root. */
int clsimhip_comm_statistics(clsimhip_comm *comm, uint64_t *gathers, double *gather_ms, uint64_t *records_sent, uint64_t *records_received, int reset);
/* Collective.  d_photons / d_hit_count: this rank's photon buffer (`capacity` records) and uint32 hit counter as
 * clsimhip_propagate_device left them.  On `root`, d_gathered (room for gathered_capacity records) receives rank 0's
 * photons, then rank 1's ...; counts_out[world_size] (host, every rank, may be NULL) receives the ranks' hit counters
 * (a rank transfers min(counter, capacity) records).  Ordered after the work already queued on `hip_stream`; returns
 * once the counts are known -- the transfers (ncclAllGather of the counts, then one ncclSend/ncclRecv per peer in one
 * group: every peer uses its own xGMI link to the root) may still be running on `hip_stream`.
 * A gather buffer that is too small for all ranks' photons: every rank learns the root's gathered_capacity with the counts,
 * the root receives the records that fit (rank 0's first), sends and receives still pair up, and EVERY rank returns
 * CLSIMHIP_ERR_ARGUMENT (counts_out is filled). */
int clsimhip_gather_hits(clsimhip_comm *comm, const void *d_photons, const void *d_hit_count, size_t capacity, int root,
                         void *d_gathered, size_t gathered_capacity, uint64_t *counts_out, void *hip_stream);

/* ---- introspection used by the parity tests ---- */
/* Which scheduling the propagation kernel runs with (after Initialize): 1 = per-wave photon pools
 * (prop_pool_kernel.hip.h), 0 = one photon per lane (prop_kernel.hip.h).  Chosen per launch: pools for bunches large
 * enough to fill them (>= 524288 steps), never with photon histories or a table image that leaves the pools no LDS.
 * Results do not depend on it.  CLSIMHIP_KERNEL=pool|classic in the environment forces one for every bunch size
 * (clsimhip_uses_pooled_kernel then reports 1 / 0), CLSIMHIP_POOL_MIN_STEPS moves the threshold. */
int clsimhip_kernel_for_bunch(const clsimhip_converter *c, size_t n_steps, int *out);
int clsimhip_uses_pooled_kernel(const clsimhip_converter *c, int *out);
/* Which of the compiled kernel instantiations the LAST launch of this converter dispatched to.  The launchers choose among
 * (lengths kind, tilt, anisotropy, flasher) x (generic, FAST) per kernel family; the report is written where the kernel is
 * launched, from that launch's own template arguments, so a test can assert that it ran the instantiation it meant to run.
 * out = {family (CLSIMHIP_FAMILY_*), lengths kind (CLSIMHIP_LENGTHS_*), tilt, anisotropy, flasher, FAST}, the last four 0 | 1;
 * every entry is -1 before the first launch.  Read-only; a launch in flight on another thread may or may not be seen yet. */
#define CLSIMHIP_FAMILY_CLASSIC 0   /* one photon per lane, STOP_PHOTONS_ON_DETECTION          */
#define CLSIMHIP_FAMILY_KEEP 1      /* one photon per lane, without STOP_PHOTONS_ON_DETECTION  */
#define CLSIMHIP_FAMILY_POOL 2      /* per-wave photon pools, STOP_PHOTONS_ON_DETECTION        */
#define CLSIMHIP_FAMILY_POOL_KEEP 3 /* per-wave photon pools, without it                       */
#define CLSIMHIP_FAMILY_TAB4 4      /* table maker, 4 axes                                     */
#define CLSIMHIP_FAMILY_TAB5 5      /* table maker, 5 axes (impact angle)                      */
int clsimhip_get_last_launch(const clsimhip_converter *c, int out[6]);
/* The pooled kernel compiled at run time for this converter's configuration ("baked_kernel" of clsimhip_set_tuning): hiprtc, loaded
 * with dlopen, compiles the
 * instantiation the launcher would take, with the values Compile() fixed as literals.  Pointers, sizes and launcher thresholds stay
 * kernel arguments.  Results are those of the precompiled kernel, bit for bit.
 * Two more keys of clsimhip_set_tuning / clsimhip_get_tuning belong to it: "baked_kernel" = 0 never; 1 (the default) for the bunches
 * the launcher itself sends to the pooled kernel, where the instantiation is the one it was measured to pay for (IceCube lengths with
 * tilt, no anisotropy, no flasher, every proof of Compile() in hand: +2.6 %; with anisotropy or a flasher it lost 1.2 - 1.4 %) -- the
 * first such launch compiles, synchronously, in about a second; 2 every instantiation, also on smaller bunches on which "kernel"
 * forced the pooled kernel (tests).  Whatever fails -- no library, a compile error, more than 80
 * vector registers or scratch in the result, a load or launch error -- runs the precompiled kernel and says so once on stderr.
 * "baked_state" (read only) is that of the last launch that asked for the kernel: 0 none yet, 1 it ran, 2 the precompiled one ran.
 * clsimhip_baked_info: state as "baked_state"; key: the module's cache key (32 hexadecimal digits + NUL; over the generated source, the
 * options, the architecture and the compiler's version); why: the reason of a fallback.  Any pointer may be null.
 * clsimhip_baked_compile (after Compile(), no GPU needed): compiles for `arch` ("gfx950") with `flags` (null: the library's own) and
 * writes the code object to code_path (may be null).  Returns 1 = compiled, 0 = not (why says it: the launches would run the
 * precompiled kernel), negative = a status.
 * clsimhip_baked_set_compiler_library: the hiprtc to load (null or "": libhiprtc.so.7, libhiprtc.so), and then no other is tried; it
 * counts until the first compilation of the process.  The library itself reads no environment variable for this; the Python binding
 * passes on CLSIMHIP_HIPRTC_LIBRARY when it loads the library. */
int clsimhip_baked_set_compiler_library(const char *path);
int clsimhip_baked_info(const clsimhip_converter *c, int *state, char key[33], char *why, size_t why_bytes);
int clsimhip_baked_compile(const clsimhip_converter *c, const char *arch, const char *flags, const char *code_path, char key[33], double *seconds,
                           char *why, size_t why_bytes);
/* copies the compiled table `name` (e.g. "geoStringPosX", "aDust400") converted to
 * double into out[0..cap); returns the entry count or a negative status.
 * "kernel_variant" (after Compile, no GPU needed): the key the launchers dispatch on, as Compile() derived it from the
 * configuration -- {lengths kind, tilt, anisotropy, flasher, without STOP_PHOTONS_ON_DETECTION, FAST proofs complete}; the
 * table maker's fifth entry is its number of axes. */
long clsimhip_get_table(const clsimhip_converter *c, const char *name, double *out, size_t cap);
/* current RNG state words (after the bunches run so far) */
int clsimhip_get_rng_state(clsimhip_converter *c, uint64_t *x_out, size_t count);
/* evaluates the device math library on the GPU: what = 0 log,1 exp,2 sin,3 cos,4 powr(x,y),
 * 5 acos,6 atan2(x,y),7 rsqrt,8 sqrt,9 x/y,10 acos (single precision),11 rcp_,12 sqrt_near_,13 rsqrt_near_,
 * 14 powr_unit_(x,y),15 cbrt_,16 div_near_(x,y) */
int clsimhip_eval_math(int device_ordinal, int what, const float *x, const float *y, size_t n, float *out);

/* Single functions of an initialised converter evaluated ON THE DEVICE, from the table image its kernels read: what the
 * reference's tester classes do (private/test/I3CLSimFunctionTester, ...ScalarFieldTester, ...VectorTransformTester,
 * ...MediumPropertiesTester, ...RandomDistributionTester; used by resources/tests/testScalarFields.py,
 * testScalarFieldIceTiltZShift.py, testVectorTransforms.py to compare device with host).  in4 / out4: n x 4 floats.
 * fast != 0: the forms the standard configuration's kernels use (exact reciprocals; only valid when Compile() proved their
 * ranges: CLSIMHIP_ERR_STATE otherwise), 0: the IEEE sequences.  Same values either way (tests/test_device_functions_gpu.py). */
#define CLSIMHIP_EVAL_LENGTHS 0                 /* in.x = wavelength [m]; out.x = absorption, out.y = scattering length of `layer` */
#define CLSIMHIP_EVAL_REFRACTION 1              /* in.x = wavelength; out.x = phase refractive index, out.y = group velocity [m/ns] */
#define CLSIMHIP_EVAL_WAVELENGTH_BIAS 2         /* in.x = wavelength; out.x = getWavelengthBias */
#define CLSIMHIP_EVAL_TILT 3                    /* in.xyz = position; out.x = getTiltZShift */
#define CLSIMHIP_EVAL_ABS_LEN_SCALING 4         /* in.xyz = direction; out.x = getDirectionalAbsLenCorrFactor */
#define CLSIMHIP_EVAL_PRE_SCATTER_TRANSFORM 5   /* in.xyz = direction; out.xyz = transformDirectionPreScatter */
#define CLSIMHIP_EVAL_POST_SCATTER_TRANSFORM 6  /* in.xyz = direction; out.xyz = transformDirectionPostScatter */
int clsimhip_eval_device_function(clsimhip_converter *c, int what, int layer, int fast, const float *in4, size_t n, float *out4);
/* n_streams work items, each with its own MWC stream (x[i], a[i]) -- x is updated --, draw `draws` values:
 * out[i * draws + k] (RandomDistributionTester.cxx:43-199) */
#define CLSIMHIP_EVAL_RANDOM_UNIFORM 0              /* rand_MWC_co */
#define CLSIMHIP_EVAL_RANDOM_WAVELENGTH 1           /* generateWavelength_<generator> */
#define CLSIMHIP_EVAL_RANDOM_SCATTERING_COSINE 2    /* makeScatteringCosAngle */
int clsimhip_eval_device_random(clsimhip_converter *c, int what, int generator, int fast, uint64_t *x, const uint32_t *a, size_t n_streams,
                                size_t draws, float *out);
/* exhaustive device-side check of the range-restricted operations of the kernel's math library (what = 11 reciprocal,
 * 12 square root, 13 reciprocal square root) against the IEEE divide / sqrt: all 2^23 significands x every binary
 * exponent in [exp_lo, exp_hi].  result[0] = number of mismatches, result[1..cap) = bit patterns of the first ones.
 * what = 16: the range-restricted divide, all 2^23 divisor significands x the divisor exponents [exp_lo, exp_hi] x both
 * divisor signs x 40 numerators each (random and adversarial, exponents -40 ... 60); result[1..] = (numerator, divisor)
 * pairs of the first mismatches.  what = 17 / 18: the reciprocal of a reciprocal, the reciprocal root next to one (detmath.hip.h).
 * what = 19: the table maker's axis bin (floor, saturating conversion, clamp: Axis.cxx:45-60) as the kernel forms it against the
 * spelled-out conversion on ALL 2^32 bit patterns x five bin counts (exp_lo / exp_hi do not apply).
 * what = 20: the run-time compiled kernel's table index from a float (unsigned conversion + minimum with the literal bound) against
 * clamp((int)f, 0, bound) on ALL 2^32 bit patterns x the bounds 0, 1, 0xa8, 0xaa, 0x1ff, 0x3fff (exp_lo / exp_hi do not apply). */
int clsimhip_check_math_exhaustive(int device_ordinal, int what, int exp_lo, int exp_hi, uint32_t *result, size_t result_cap);

const char *clsimhip_version(void);

/* ---- step producer on the GPU (the arithmetic that is part of the reference tree) ----------
 * One request = one entry of the reference's step generation queue (CascadeStepData_t / MuonStepData_t,
 * private/clsim/I3CLSimLightSourceToStepConverterPPC.h): the particle, how many steps of how many photons it was
 * given (I3CLSimLightSourceToStepConverterPPC.cxx:284-470 computes those from sim-services / GSL / the random
 * service -- not part of this library), and the longitudinal profile parameters.  Steps are generated like
 * FillStep/GenerateStep/GenerateStepForMuon (:524-551, :785-842) do, one GPU lane per step. */
#define CLSIMHIP_STEPS_CASCADE 0        /* CascadeStepData_t: position = pb * Gamma(pa) along the axis, PPC angular profile */
#define CLSIMHIP_STEPS_MUON_CASCADE 1   /* MuonStepData_t, stepIsCascadeLike: position uniform along `length`, angular profile */
#define CLSIMHIP_STEPS_MUON 2           /* MuonStepData_t, muon-like: every step is the whole track (length, direction) */
typedef struct {
    float x, y, z, time;                /* particle vertex [m, ns] */
    float dx, dy, dz;                   /* unit direction of flight */
    float length;                       /* MUON*: track length [m] */
    float pa, pb;                       /* CASCADE: shower_params.a, shower_params.b [m] (b = 0: no cascade extension) */
    uint32_t kind;
    uint32_t identifier;                /* -> I3CLSimStep::identifier */
    uint32_t photons_per_step;
    uint32_t num_photons_in_last_step;  /* a last step with this many photons is appended when > 0 */
    uint64_t num_steps;                 /* steps of photons_per_step photons */
} clsimhip_step_request;
/* steps the requests produce; *padded_out = that number rounded up to a multiple of `granularity` (the converter's
 * workgroup size) with the reference's no-op steps (Async.cxx:240-257) */
int clsimhip_count_generated_steps(const clsimhip_step_request *requests, size_t n, size_t granularity,
                                   size_t *steps_out, size_t *padded_out);
/* generates into device memory d_steps (room for `capacity` steps) on `hip_stream`; asynchronous */
int clsimhip_generate_steps_device(int device, const clsimhip_step_request *requests, size_t n, uint64_t seed,
                                   size_t granularity, void *d_steps, size_t capacity, void *hip_stream, size_t *padded_out);
/* the same into host memory (synchronous) */
int clsimhip_generate_steps(int device, const clsimhip_step_request *requests, size_t n, uint64_t seed,
                            size_t granularity, clsimhip_step *steps_out, size_t capacity, size_t *padded_out);

/* ---- particle -> step requests: the front end of I3CLSimLightSourceToStepConverterPPC ----------
 * private/clsim/I3CLSimLightSourceToStepConverterPPC.cxx, Initialize :94-132 (photon yield per metre of track,
 * ConverterUtils.cxx:44-105) and EnqueueLightSource :188-470: 5.21 m of Cherenkov-radiating track per GeV (scaled with the
 * density), the electromagnetic fraction of hadronic showers with its fluctuation, a Poisson (Gaussian above 1e7) number
 * of photons, the split into steps of photonsPerStep (highPhotonsPerStep above a threshold) photons; muons and taus as
 * a bare track plus the average secondary light (1 + max(0, 0.1880 + 0.0206 ln E)).  Host only.
 * NOT part of the reference tree and therefore restated from published sources, PARITY UNPINNED:
 * I3SimConstants::ShowerParameters (sim-services), the random service's Gaus / Poisson (phys-services / GSL), and
 * gsl_integration_qag.  Particle types are I3Particle::ParticleType values (dataclasses): PDG codes, and IceCube's own
 * codes for stochastic losses. */
#define CLSIMHIP_PARTICLE_GAMMA 22
#define CLSIMHIP_PARTICLE_EMINUS 11
#define CLSIMHIP_PARTICLE_EPLUS (-11)
#define CLSIMHIP_PARTICLE_MUMINUS 13
#define CLSIMHIP_PARTICLE_MUPLUS (-13)
#define CLSIMHIP_PARTICLE_TAUMINUS 15
#define CLSIMHIP_PARTICLE_TAUPLUS (-15)
#define CLSIMHIP_PARTICLE_PI0 111
#define CLSIMHIP_PARTICLE_PIPLUS 211
#define CLSIMHIP_PARTICLE_PIMINUS (-211)
#define CLSIMHIP_PARTICLE_K0_LONG 130
#define CLSIMHIP_PARTICLE_KPLUS 321
#define CLSIMHIP_PARTICLE_KMINUS (-321)
#define CLSIMHIP_PARTICLE_K0_SHORT 310
#define CLSIMHIP_PARTICLE_PPLUS 2212
#define CLSIMHIP_PARTICLE_PMINUS (-2212)
#define CLSIMHIP_PARTICLE_NEUTRON 2112
#define CLSIMHIP_PARTICLE_BREMS (-2000001001)
#define CLSIMHIP_PARTICLE_DELTAE (-2000001002)
#define CLSIMHIP_PARTICLE_PAIRPROD (-2000001003)
#define CLSIMHIP_PARTICLE_NUCLINT (-2000001004)
#define CLSIMHIP_PARTICLE_HADRONS (-2000001006)
#define CLSIMHIP_SHAPE_OTHER 0
#define CLSIMHIP_SHAPE_CASCADE_SEGMENT 1        /* I3Particle::CascadeSegment: steps spread uniformly over `length` (:342-357) */
typedef struct {
    int32_t type;                       /* CLSIMHIP_PARTICLE_* / any PDG code (unknown codes are treated as hadrons, :272-279) */
    int32_t shape;                      /* CLSIMHIP_SHAPE_* */
    double x, y, z, time;               /* [m, ns] */
    double dx, dy, dz;                  /* unit direction */
    double energy;                      /* [GeV] */
    double length;                      /* [m]; NaN: unknown (muons then get 2000 m, :377-380) */
    uint32_t identifier;                /* -> I3CLSimStep::identifier of its steps */
    uint32_t reserved;
} clsimhip_particle;
typedef struct {
    uint32_t photons_per_step;          /* photonsPerStep (200) */
    uint32_t high_photons_per_step;     /* highPhotonsPerStep (2000) */
    double use_high_photons_per_step_from;  /* useHighPhotonsPerStepStartingFromNumPhotons (1e9) */
    int32_t use_cascade_extension;      /* UseCascadeExtension (on) */
    int32_t reserved;
    double medium_density;              /* g/cm3; I3CLSimMediumProperties::GetMediumDensity(), 0.9216 for the IceCube media */
    uint64_t seed;                      /* of this library's generator (in the place of the I3RandomService) */
} clsimhip_ppc_config;
typedef struct clsimhip_ppc_converter clsimhip_ppc_converter;
/* SetWlenBias + SetMediumProperties + Initialize */
int clsimhip_ppc_create(const clsimhip_medium *medium, const clsimhip_function *wavelength_bias, const clsimhip_ppc_config *config,
                        clsimhip_ppc_converter **out);
void clsimhip_ppc_destroy(clsimhip_ppc_converter *p);
/* meanPhotonsPerMeterInLayer_[layer] (beta = 1, after the wavelength bias) */
int clsimhip_ppc_photons_per_meter(const clsimhip_ppc_converter *p, int layer, double *out);
/* EnqueueLightSource for n particles: one request per cascade, two per muon / tau (muon-like, then cascade-like steps),
 * ready for clsimhip_generate_steps[_device].  *n_out = requests the particles need; at most `capacity` are written. */
int clsimhip_ppc_enqueue(const clsimhip_ppc_converter *p, const clsimhip_particle *particles, size_t n,
                         clsimhip_step_request *requests_out, size_t capacity, size_t *n_out);
/* I3SimConstants::ShowerParameters as restated here: out = {a, b [m], emScale, emScaleSigma} */
int clsimhip_shower_parameters(int32_t particle_type, double energy_gev, double density_g_cm3, double out[4]);

/* ---- flasher step producer --------------------------------------------------------------
 * I3CLSimLightSourceToStepConverterFlasher (private/clsim/I3CLSimLightSourceToStepConverterFlasher.cxx): MakeSteps
 * :329-440 cuts a flasher pulse into steps of photons_per_step photons (zero length, beta 1, weight 1, the pulse's
 * spectrum as source type) and pads with dummy steps to the bunch granularity; FillStep :443-545 smears every step's
 * direction and time with three I3CLSimRandomValue distributions whose run-time parameter comes from the pulse.
 * One GPU lane makes one step, every step has its own MWC stream seeded from (seed, step index) -- the reference
 * samples with I3RandomService (phys-services, not part of the reference tree) in double precision, so parity is
 * product = oracle (oracle/stepgen_oracle.c) and distribution tests, as for the cascade/muon producer.
 * Kept from the reference: a pulse whose photons divide evenly into more than one step loses its last step to a
 * dummy step (:383-389 with :407-408). */
#define CLSIMHIP_DIST_CONSTANT 0                /* I3CLSimRandomValueConstant(): the run-time parameter itself */
#define CLSIMHIP_DIST_NORMAL 1                  /* FixParameter(NormalDistribution(), 0, value): value + parameter * Box-Muller
                                                   (random_value/I3CLSimRandomValueNormalDistribution.cxx:47-80) */
#define CLSIMHIP_DIST_UNIFORM 2                 /* Uniform(value, NaN): value + u * (parameter - value) (…Uniform.cxx:77-104) */
#define CLSIMHIP_DIST_FLASHER_TIME_PROFILE 3    /* python/I3CLSimRandomValueIceCubeFlasherTimeProfile.py: LED pulse shape for
                                                   the pulse width (parameter), an InterpolatedDistribution of 240 points */
typedef struct {
    int32_t kind;
    float value;                                /* NORMAL: mean; UNIFORM: from */
} clsimhip_distribution;
typedef struct {
    clsimhip_distribution polar;                /* angularProfileDistributionPolar, parameter = sigma_polar */
    clsimhip_distribution azimuthal;            /* angularProfileDistributionAzimuthal, parameter = sigma_azimuthal */
    clsimhip_distribution time_delay;           /* timeDelayDistribution, parameter = pulse_width */
    int32_t interpret_in_polar_coordinates;     /* interpretAngularDistributionsInPolarCoordinates (:497-541) */
    uint32_t photons_per_step;                  /* photonsPerStep_ (default 400, :46) */
    uint32_t max_bunch_size;                    /* maxBunchSize_ (default 512000, :47) */
    uint32_t bunch_size_granularity;            /* bunchSizeGranularity_ (default 512, :48) */
} clsimhip_flasher_config;
typedef struct {                                /* one I3CLSimFlasherPulse in the converter's queue (LightSourceData_t) */
    float x, y, z, time;
    float dx, dy, dz;                           /* GetDir(), direction of emission */
    float sigma_polar, sigma_azimuthal;         /* GetAngularEmissionSigmaPolar / Azimuthal [rad] */
    float pulse_width;                          /* GetPulseWidth [ns] */
    uint32_t identifier;
    uint32_t source_type;                       /* spectrumSourceTypeIndex_: wavelength generator of the pulse's spectrum */
    uint64_t num_photons_with_bias;             /* numPhotonsWithBias (EnqueueLightSource :243-262, computed by the caller) */
} clsimhip_flasher_request;                     /* 56 bytes */
/* The converter's front end (Initialize :120-159, EnqueueLightSource :214-265): photons after the wavelength bias =
 * GetNumberOfPhotonsNoBias() x PhotonNumberCorrectionFactorAfterBias (ConverterUtils.cxx:113-214: the bias at the peak for a
 * delta-peak spectrum -- spectrum_no_bias NULL, peak_wavelength used -- else the ratio of the spectrum's integrals with and
 * without bias over [from, to]), then Poisson, or a non-negative Gaussian above 1e6; pulses that end up without photons
 * are skipped.  The random numbers are this library's (one counter-based stream per identifier), as for clsimhip_ppc_*. */
typedef struct {
    float x, y, z, time;
    float dx, dy, dz;
    float sigma_polar, sigma_azimuthal;
    float pulse_width;
    uint32_t identifier;
    uint32_t source_type;
    double num_photons_no_bias;                 /* I3CLSimFlasherPulse::GetNumberOfPhotonsNoBias() */
} clsimhip_flasher_pulse;
int clsimhip_flasher_correction_factor(const clsimhip_function *spectrum_no_bias, double peak_wavelength,
                                       const clsimhip_function *wavelength_bias, double from_wavelength, double to_wavelength, double *out);
int clsimhip_flasher_enqueue(double correction_factor, uint64_t seed, const clsimhip_flasher_pulse *pulses, size_t n,
                             clsimhip_flasher_request *requests_out, size_t capacity, size_t *n_out);
/* number of output steps (real + dummy) and of steps that carry photons */
int clsimhip_count_flasher_steps(const clsimhip_flasher_config *config, const clsimhip_flasher_request *requests, size_t n,
                                 size_t *steps_out, size_t *real_steps_out);
/* generates into device memory d_steps (room for `capacity` steps) on `hip_stream` */
int clsimhip_generate_flasher_steps_device(int device, const clsimhip_flasher_config *config, const clsimhip_flasher_request *requests,
                                           size_t n, uint64_t seed, void *d_steps, size_t capacity, void *hip_stream, size_t *steps_out);
/* the same into host memory (synchronous) */
int clsimhip_generate_flasher_steps(int device, const clsimhip_flasher_config *config, const clsimhip_flasher_request *requests,
                                    size_t n, uint64_t seed, clsimhip_step *steps_out, size_t capacity, size_t *count_out);
/* the time delay distribution for one pulse width: 240 densities and cumulative values at 0.5 ns spacing (host only) */
int clsimhip_flasher_time_profile(double pulse_width_ns, float density[240], float cumulative[240]);

/* ---- step store ------------------------------------------------------------------------
 * I3CLSimStepStore (public/clsim/I3CLSimStepStore.h:44-320): steps sorted by photon count (one FIFO per count), with
 * the number of stored steps per identifier; the feeder thread of the reference cuts bunches from it
 * (I3CLSimLightSourceToStepConverterAsync.cxx:209-273).  Host memory only. */
typedef struct clsimhip_step_store clsimhip_step_store;
int clsimhip_step_store_create(size_t initial_bins, clsimhip_step_store **out);
void clsimhip_step_store_destroy(clsimhip_step_store *s);
/* insert_copy(step.GetNumPhotons(), step) for n steps (StepStore.h:266-283) */
int clsimhip_step_store_insert(clsimhip_step_store *s, const clsimhip_step *steps, size_t n);
int clsimhip_step_store_size(const clsimhip_step_store *s, size_t *out);
/* count(identifier) (StepStore.h:308-312) */
int clsimhip_step_store_count(const clsimhip_step_store *s, uint32_t identifier, uint32_t *out);
/* pop_bunch_to_vector(size, vect): ascending photon count, FIFO within a count; *popped <= size (StepStore.h:163-198) */
int clsimhip_step_store_pop_bunch(clsimhip_step_store *s, size_t size, clsimhip_step *out, size_t *popped);
/* pop_bunch_to_vector(size, vect, temp): exactly `size` steps, the remainder copies of *fill (StepStore.h:209-222) */
int clsimhip_step_store_pop_bunch_filled(clsimhip_step_store *s, size_t size, clsimhip_step *out, const clsimhip_step *fill);
/* numStepsWithDummyFill (Async.cxx:256): size of the padded last bunch before a barrier */
int clsimhip_step_store_size_with_dummy_fill(const clsimhip_step_store *s, size_t granularity, size_t *out);

/* ---- feeder: the worker thread of I3CLSimLightSourceToStepConverterAsync ----------------------
 * private/clsim/I3CLSimLightSourceToStepConverterAsync.cxx: EnqueueLightSource / EnqueueBarrier / BarrierActive /
 * MoreStepsAvailable / GetConversionResultWithBarrierInfo (:470-600) in front of WorkerThread_impl (:178-392): light sources
 * are converted one after the other (the PPC front end above + the GPU step producer take the place of the
 * parameterisation), their steps go through the step store, and bunches of max_bunch_size steps come out in ascending
 * photon count, each with the identifiers of the light sources that have completely left the store; the barrier flushes
 * the rest, padded with no-op steps to ((size / granularity) + 1) * granularity.  Queues of `queue_depth` entries (10 in
 * the reference) on both sides; one thread per feeder. */
typedef struct clsimhip_feeder clsimhip_feeder;
/* ppc may be NULL (only clsimhip_feeder_enqueue_steps is then accepted); it must outlive the feeder */
int clsimhip_feeder_create(const clsimhip_ppc_converter *ppc, int device, uint64_t seed, size_t max_bunch_size,
                           size_t bunch_size_granularity, size_t queue_depth, clsimhip_feeder **out);
void clsimhip_feeder_destroy(clsimhip_feeder *f);
int clsimhip_feeder_enqueue_light_source(clsimhip_feeder *f, const clsimhip_particle *particle);
/* a light source whose steps the caller made itself (the role of an I3CLSimLightSourcePropagator, e.g. Geant4) */
int clsimhip_feeder_enqueue_steps(clsimhip_feeder *f, uint32_t identifier, const clsimhip_step *steps, size_t n);
int clsimhip_feeder_enqueue_barrier(clsimhip_feeder *f);
int clsimhip_feeder_barrier_active(const clsimhip_feeder *f, int *out);
int clsimhip_feeder_more_steps_available(const clsimhip_feeder *f, int *out);
/* GetConversionResultWithBarrierInfoAndMarkers: waits up to timeout_ms (< 0: for ever; *got = 0 on timeout).  *steps (n
 * records) and *finished (n_finished identifiers) stay valid until clsimhip_feeder_release_result(f, *steps). */
int clsimhip_feeder_get_conversion_result(clsimhip_feeder *f, double timeout_ms, int *got, const clsimhip_step **steps, size_t *n,
                                          const uint32_t **finished, size_t *n_finished, int *barrier_was_reset);
int clsimhip_feeder_release_result(clsimhip_feeder *f, const clsimhip_step *steps);

/* ---- photon table maker -------------------------------------------------------------
 * I3CLSimStepToTableConverter (private/clsim/tabulator/I3CLSimStepToTableConverter.h:44-101): propagates steps with
 * the TABULATE variant of propKernel (propagation_kernel.c.cl:228-303, 755-785: fixed 42 absorption lengths, no
 * detector, a path sample every `step_length` metres) and fills a table over coordinates relative to a reference
 * particle.  4 axes, or 5 = TABULATE_IMPACT_ANGLE (StepToTableConverter.cxx:187-188: the fifth axis is the cosine of
 * the impact angle on the DOM, two random numbers per path sample); linear and power axes (inverse transform: sqrt, cbrt,
 * pow(x, 1/power), tabulator/Axis.cxx:150-171). */
#define CLSIMHIP_AXIS_LINEAR 0          /* clsim::tabulator::LinearAxis (tabulator/Axis.h:71-80) */
#define CLSIMHIP_AXIS_POWER 1           /* clsim::tabulator::PowerAxis  (tabulator/Axis.h:82-95) */
typedef struct {
    int32_t kind;
    double min, max;
    uint32_t n_bins;                    /* without the under-/overflow bins every axis gets (Axes.cxx:51-64) */
    uint32_t power;                     /* POWER: >= 1 (2: square-root spacing, 3: cube-root ...) */
} clsimhip_axis;
#define CLSIMHIP_AXES_SPHERICAL 0       /* SphericalAxes: r, azimuth [deg], cos(polar), delay time (spherical_coordinates.c.cl) */
#define CLSIMHIP_AXES_CYLINDRICAL 1     /* CylindricalAxes: rho, azimuth [rad], z, delay time (cylindrical_coordinates.c.cl) */
typedef struct {                        /* I3CLSimFunctionPolynomial (function/I3CLSimFunctionPolynomial.cxx:35-153) */
    int32_t n;
    const double *coefficients;         /* c0 + c1 x + c2 x^2 + ...  Two users, two evaluation orders: the table maker's kernel
                                           evaluates it in single precision in Horner form, c0 + x*(c1 + x*(...)), as the OpenCL
                                           text the reference generates does (Polynomial.cxx:104-153); the MCPE generator below
                                           follows the host GetValue (:85-101) in double precision: sum += c_i * multiplier,
                                           multiplier *= x */
    double range_min, range_max;        /* -inf / +inf: unbounded */
    double underflow, overflow;
} clsimhip_polynomial;
typedef struct clsimhip_tabulator clsimhip_tabulator;

/* I3CLSimStepToTableConverter::I3CLSimStepToTableConverter (StepToTableConverter.cxx:122-265).  wavelength_acceptance
 * biases the Cherenkov spectrum (generator 0) and weights nothing else; angular_acceptance is evaluated on the
 * photon's z direction cosine per path segment; reference_area and step_length enter Normalize().  (x, a): one MWC
 * stream per work item, `streams` a multiple of 256. */
int clsimhip_tabulator_create(int device, int axes_kind, const clsimhip_axis *axes, size_t n_axes, int store_squared_weights,
                              const clsimhip_medium *medium, const clsimhip_function *wavelength_acceptance,
                              const clsimhip_polynomial *angular_acceptance, double reference_area, double step_length,
                              const uint64_t *x, const uint32_t *a, size_t streams, clsimhip_tabulator **out);
void clsimhip_tabulator_destroy(clsimhip_tabulator *t);
const char *clsimhip_tabulator_last_error(const clsimhip_tabulator *t);
/* EnqueueSteps(steps, reference) (:272-285): reference = {x, y, z, time, dx, dy, dz} of the source particle.
 * Asynchronous; stream i of this bunch continues where stream i of the previous bunch stopped. */
int clsimhip_tabulator_enqueue_steps(clsimhip_tabulator *t, const clsimhip_step *steps, size_t n, const double reference[7]);
/* Finish() (:287-295): waits until every enqueued bunch is in the table */
int clsimhip_tabulator_finish(clsimhip_tabulator *t);
/* table maker tuning (see clsimhip_set_tuning; no result depends on it): "fast_kernels" 0 | 1 -- the instantiation with the
 * medium's proofs compiled in, measured slower for this kernel (0); "grid" -- workgroups of the launch, 0: automatic (0);
 * "standard_sampler" 0 | 1 -- 0: the generic path sampler also for a table of the reference's default shape (spherical, folded
 * azimuth, square-root distance and time axes, no squared weights), which otherwise runs the sampler specialised for it (1) */
int clsimhip_tabulator_set_tuning(clsimhip_tabulator *t, const char *key, long long value);
/* number of bins including under-/overflow bins, number of axes (4, or 5 with the impact angle), and the shape
 * (n_bins + 2 per axis; unused entries 0) */
int clsimhip_tabulator_get_shape(const clsimhip_tabulator *t, size_t *n_bins, size_t *n_dim, size_t shape[5]);
/* binContent_ (squared == 0) or squaredWeights_ as the float image WriteFITSFile stores (:595-686), before
 * (normalized == 0) or after Normalize() (:512-543) */
int clsimhip_tabulator_get_bin_content(clsimhip_tabulator *t, float *out, size_t n_bins, int squared, int normalized);
/* the double precision accumulators themselves */
int clsimhip_tabulator_get_bin_sums(clsimhip_tabulator *t, double *out, size_t n_bins, int squared);
/* Axis::GetBinEdges (Axis.cxx:62-74): n_bins + 1 edges of axis `axis` */
int clsimhip_tabulator_get_bin_edges(const clsimhip_tabulator *t, int axis, double *out, size_t cap);
/* [0] photons enqueued, [1] sum of photon weights (numPhotons*weight), [2] n_group, [3] n_phase of
 * GetMinimumRefractiveIndex (:96-120), [4] kernel time ms, [5] launches, [6] bins, [7] reserved */
int clsimhip_tabulator_get_statistics(clsimhip_tabulator *t, double out[8]);
/* WriteFITSFile(path, tableHeader) (:595-686): normalised bin content as the primary image (axis counts reversed, as
 * cfitsio/PyFITS store it), "HIERARCH _i3_<key>" header keywords -- n_photons (= spectralBiasFactor x sum of photon
 * weights), n_group, n_phase, then the caller's n_keys entries (is_int[i] ? int_values[i] : double_values[i]) --, the
 * squared weights as the IMAGE extension "ERRORS", one double IMAGE extension "EDGESi" per axis.  Written without cfitsio;
 * refuses to overwrite an existing file, like fits_create_diskfile. */
int clsimhip_tabulator_write_fits_file(clsimhip_tabulator *t, const char *path, const char *const *keys, const int32_t *is_int,
                                       const int64_t *int_values, const double *double_values, size_t n_keys);
int clsimhip_tabulator_get_rng_state(clsimhip_tabulator *t, uint64_t *x, size_t count);
long clsimhip_tabulator_get_table(const clsimhip_tabulator *t, const char *name, double *out, size_t cap);
/* the instantiation of the table maker's last launch: out as clsimhip_get_last_launch (family TAB4 or TAB5, flasher always 1) */
int clsimhip_tabulator_get_last_launch(const clsimhip_tabulator *t, int out[6]);

/* ---- MCPE generator: detected photons -> photo-electrons (no device counterpart in the reference) --------------------
 * The stage behind the propagator: I3CLSimPhotonToMCPEConverterForDOMs::Convert (private/clsim/dom/
 * I3PhotonToMCPEConverter.cxx:602-669), which the reference's client module calls for every returned photon on a host thread
 * (I3CLSimClientModule.cxx:359-439), with the arrival time correction of the older module in the same file (:512-518; zero when
 * pancake = oversize).  A pure function of one delivered photon record (string and OM IDs in it, not indices), a fixed
 * configuration and a 64-bit seed:
 *     weight < 0 -> NEGATIVE_WEIGHT; weight == 0 -> no MCPE; the photon is not within 3 cm of the radius dom_radius * oversize /
 *     pancake -> OFF_SURFACE; P = weight x wavelength acceptance of the DOM's class x angular acceptance(-direction z, clamped
 *     to [-1, 1]); no class for the DOM -> UNKNOWN_DOM; P > 1 -> PROBABILITY_ABOVE_ONE; an MCPE when P > u,
 *     u = (h >> 11) 2^-53, h = seed folded with splitmix64 over the record's ten 64-bit words;
 *     time = photon time + (-position . direction) (1 - pancake / oversize) / group velocity.
 * All of it is binary64 + - x / in one fixed order (the two sin / cos pairs of the direction: the library's deterministic single
 * precision ones), so the HIP kernel and the host twin give the same bits -- for every 80-byte pattern, physical or not:
 *     angles: any float.  Outside [0, 2 pi] the sin / cos pair reduces by multiples of pi / 2 with a quadrant count held in an int32;
 *     where the count does not fit (|angle| from about 3.37e9, infinities) it saturates to INT32_MAX / INT32_MIN, for a NaN it is 0
 *     (what gfx950's conversion gives; the twin says so explicitly).  Such a direction is meaningless but defined: finite garbage for a
 *     huge angle, NaNs for an infinite or NaN angle, and a NaN -direction z clamps to 1;
 *     comparisons with a NaN are false: a NaN weight, acceptance or P passes both P > 1 and P <= u and yields an MCPE, a NaN r^2 is
 *     OFF_SURFACE, a NaN wavelength reads the table's last bin; float32 denormals are kept (nothing is flushed);
 *     time: the formula's value, infinities included; a NaN, however it came about (a NaN photon time or group velocity, 0 / 0 from
 *     a zero group velocity with pancake = oversize, inf - inf), is stored as the one pattern 0x7ff8000000000000.
 * The reference draws u from an I3RandomService in
 * arrival order, which no two runs repeat; keying the draw on the record makes the result independent of the schedule and
 * takes nothing from the propagator's RNG streams.  The four named conditions are log_fatal in the reference. */
typedef struct {                        /* I3MCPE(particle, npe = 1, time); the particle's major / minor ID and time shift are */
    uint32_t identifier;                /* the caller's, keyed by `identifier` (AddPhotonsToFrames, ClientModule.cxx:359-439)   */
    int16_t string_id;
    uint16_t om_id;
    double time;
} clsimhip_mcpe;                        /* 16 bytes */
#define CLSIMHIP_MCPE_NEGATIVE_WEIGHT 0         /* index into the condition counters */
#define CLSIMHIP_MCPE_OFF_SURFACE 1
#define CLSIMHIP_MCPE_UNKNOWN_DOM 2
#define CLSIMHIP_MCPE_PROBABILITY_ABOVE_ONE 3
typedef struct clsimhip_mcpe_generator clsimhip_mcpe_generator;
/* n_classes (1 ... 8) wavelength acceptances, kinds TABLE and CONSTANT (others: CLSIMHIP_ERR_CONFIG; at most 4096 table values
 * together), the class of every DOM as parallel arrays (the reference's I3CLSimFunctionMap: IceCube / DeepCore,
 * python/traysegments/common.py:185-210; at most 2^24 DOMs), the angular acceptance (at most 32 coefficients).  Host only: no
 * GPU is touched. */
int clsimhip_mcpe_generator_create(const clsimhip_function *classes, size_t n_classes, size_t n_doms, const int32_t *string_ids,
                                   const uint32_t *om_ids, const int32_t *class_index, const clsimhip_polynomial *angular_acceptance,
                                   double dom_radius, double oversize, double pancake, uint64_t seed, clsimhip_mcpe_generator **out);
/* a converter the generator was given to keeps it alive until the converter is destroyed */
void clsimhip_mcpe_generator_destroy(clsimhip_mcpe_generator *g);
const char *clsimhip_mcpe_generator_last_error(const clsimhip_mcpe_generator *g);
/* The host twin: the definition, for callers without a GPU and for the tests.  Keeps the input order.  *n_out = MCPEs made (may
 * exceed `capacity`: only the first `capacity` are stored); counters[4] (may be NULL) receives the four condition counts. */
int clsimhip_mcpe_convert_host(const clsimhip_mcpe_generator *g, const clsimhip_photon *photons, size_t n, clsimhip_mcpe *out,
                               size_t capacity, size_t *n_out, uint64_t counters[4]);
/* The kernel, on records that live in HBM (pairs with clsimhip_propagate_device + index -> ID conversion, or any buffer of records
 * with IDs): min(*d_hit_count, capacity) records of d_photons (16-byte aligned).  d_counters: five uint32, zeroed by this call;
 * [0] counts the MCPEs and keeps counting past mcpe_capacity (only the first mcpe_capacity are stored in d_mcpes, the photon
 * counter's rule), [1..4] the four conditions.  Output order is unspecified.  Asynchronous on hip_stream (NULL = default stream). */
int clsimhip_mcpe_convert_device(clsimhip_mcpe_generator *g, int device, const void *d_photons, const void *d_hit_count, size_t capacity,
                                 void *d_mcpes, size_t mcpe_capacity, void *d_counters, void *hip_stream);
/* Attach the generator to a converter: the kernel then runs on every bunch's stream behind the propagation kernels, over the
 * records the bunch stored.  Before Initialize() only (CLSIMHIP_ERR_STATE after); g = NULL switches it off (the default).
 * Compile() then refuses (CLSIMHIP_ERR_CONFIG) a geometry with a DOM that has no class or whose IDs do not fit the record, a
 * generator made for another pancake factor than the converter's (its records would all be OFF_SURFACE), and photon histories
 * together with keep_photons = 0 (a history belongs to a photon record).
 * keep_photons != 0: results carry the photons as without a generator, plus MCPEs.
 * keep_photons = 0: the photon records never cross to the host; a result's photon count is 0 and its `photons` pointer is a
 * non-NULL handle for clsimhip_get_result_mcpes / clsimhip_release_result (the client module's two switches). */
int clsimhip_set_mcpe_generator(clsimhip_converter *c, clsimhip_mcpe_generator *g, int keep_photons);
/* MCPEs of the result `photons` belongs to; valid until clsimhip_release_result(c, photons).  *mcpes is NULL when there are none.
 * A bunch that met one of the four conditions fails as a bunch with a corrupted record does (the worker stops,
 * CLSIMHIP_ERR_DEVICE with the four counts in the text). */
int clsimhip_get_result_mcpes(clsimhip_converter *c, const clsimhip_photon *photons, const clsimhip_mcpe **mcpes, size_t *n);

/* ---- MCPE series: a bunch's MCPEs as per-frame, per-DOM time-sorted series ---------------------------------------------
 * What the reference's client module does with every MCPE on a host thread before a frame receives its I3MCPESeriesMap:
 * AddPhotonsToFrames (private/clsim/I3CLSimClientModule.cxx:359-439: particle cache lookup, ignoreModules, time shift,
 * (*frame->hits)[omkey]) and the per-DOM time order (private/clsim/dom/I3PhotonToMCPEConverter.cxx:524-526), as a sorting stage
 * behind the MCPE kernel.  Per record, in this order:
 *     its DOM is not one of the generator's -> UNKNOWN_DOM, no record (the generator's own MCPEs never meet this);
 *     its identifier is not in the particle table -> UNKNOWN_PARTICLE, no record (log_fatal in the reference, :388-390);
 *     (frame, string_id, om_id) is in the mask -> MASKED, no record (:399; not an error);
 *     time' = time + time_shift, one binary64 addition (:334; without a table the shift is +0.0, which turns -0.0 into +0.0).
 * The kept records come out ascending in the integer key (frame, DOM rank, tkey, identifier): frames in ascending frame ID, DOMs
 * in ascending (string_id signed, om_id) -- OMKey::operator< with PMT 0 --, and b = bits(time'), tkey = b ^ (b >> 63 ? ~0 :
 * 1 << 63), a total order on bit patterns (-0.0 before +0.0, negative NaNs before -inf, positive NaNs after +inf; nothing depends
 * on < of doubles).  Records with equal keys are byte-identical, so the output is a function of the input as a multiset: the same
 * bytes from run to run, whatever the schedule, and the same bytes from the kernels and the host twin.  The series table has one
 * entry per non-empty (frame, DOM) in the same order; its entries partition the records.
 * The reference adds the shift to the photon's time before the conversion, in the photon's precision; here it is added once, after
 * the arrival time correction, in binary64.  Hit merging and the particle-ID map are the next stage ("MCPE merging"
 * below). */
typedef struct {                        /* one entry of the particle cache: the frame the particle belongs to and its time shift */
    uint32_t identifier;                /* strictly increasing over the table (CLSIMHIP_ERR_ARGUMENT otherwise) */
    uint32_t frame;                     /* the caller's frame ID, any value */
    double time_shift;
} clsimhip_mcpe_particle;               /* 16 bytes */
typedef struct {                        /* one module of one frame's ignoreModules; entries that name a frame or a DOM the bunch */
    uint32_t frame;                     /* never meets are ignored */
    int16_t string_id;
    uint16_t om_id;
} clsimhip_mcpe_mask;                   /* 8 bytes */
typedef struct {
    uint32_t frame;
    int16_t string_id;
    uint16_t om_id;
    uint32_t first, count;              /* records [first, first + count) */
} clsimhip_mcpe_series;                 /* 16 bytes */
typedef char clsimhip_mcpe_is_16_bytes[sizeof(clsimhip_mcpe) == 16 ? 1 : -1];
typedef char clsimhip_mcpe_particle_is_16_bytes[sizeof(clsimhip_mcpe_particle) == 16 ? 1 : -1];
typedef char clsimhip_mcpe_series_is_16_bytes[sizeof(clsimhip_mcpe_series) == 16 ? 1 : -1];
typedef char clsimhip_mcpe_mask_is_8_bytes[sizeof(clsimhip_mcpe_mask) == 8 ? 1 : -1];
#define CLSIMHIP_SERIES_UNKNOWN_PARTICLE 0      /* index into the series counters */
#define CLSIMHIP_SERIES_MASKED 1
#define CLSIMHIP_SERIES_UNKNOWN_DOM 2
/* The host twin: the definition with std::sort on the key, for callers without a GPU and for the tests.  `g` supplies the DOM
 * list.  particles = NULL, n_particles = 0: no table -- every identifier belongs to frame 0 with shift 0.  out and series hold n
 * entries each; counters[3] (may be NULL) receives the three counts.  CLSIMHIP_ERR_CONFIG when frames x DOMs >= 2^32. */
int clsimhip_mcpe_series_host(const clsimhip_mcpe_generator *g, const clsimhip_mcpe *mcpes, size_t n, const clsimhip_mcpe_particle *particles,
                              size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked, clsimhip_mcpe *out,
                              clsimhip_mcpe_series *series, size_t *n_kept, size_t *n_series, uint64_t counters[3]);
/* bytes of device memory the kernels need beside their input and output, for up to `capacity` records and a bunch with this table
 * and mask */
size_t clsimhip_mcpe_series_workspace_bytes(size_t capacity, size_t n_particles, size_t n_masked);
/* The kernels, on MCPEs that live in HBM (pairs with clsimhip_mcpe_convert_device: d_mcpes and d_count = its d_counters, whose
 * first word counts past the capacity): min(*d_count, capacity) records of d_mcpes.  d_out and d_series: `capacity` entries each,
 * d_workspace: clsimhip_mcpe_series_workspace_bytes(capacity, n_particles, n_masked) bytes, all 16-byte aligned; d_counts: five
 * uint32 -- records kept, series, then the three counters.  The particle table and the mask are host memory: they are checked and
 * copied before the call returns (which may wait for the previous call's copy, nothing else); the kernels are asynchronous on
 * hip_stream (NULL = default stream) and nothing else waits for the device. */
int clsimhip_mcpe_series_device(clsimhip_mcpe_generator *g, int device, const void *d_mcpes, const void *d_count, size_t capacity,
                                const clsimhip_mcpe_particle *particles, size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked,
                                void *d_out, void *d_series, void *d_counts, void *d_workspace, size_t workspace_bytes, void *hip_stream);
/* The stage behind every bunch's MCPE kernel, on the bunch's stream.  Before Initialize() only (CLSIMHIP_ERR_STATE after);
 * Compile() refuses it without an MCPE generator (CLSIMHIP_ERR_CONFIG).  on = 0 (the default): nothing changes anywhere.
 * With it on, clsimhip_get_result_mcpes returns the sorted records, and a bunch with UNKNOWN_PARTICLE (or UNKNOWN_DOM) > 0 fails
 * as a bunch with one of the MCPE generator's four conditions does, with the count in the text. */
int clsimhip_set_mcpe_series(clsimhip_converter *c, int on);
/* clsimhip_enqueue_steps with the bunch's particle table and mask, which are checked and copied in the caller's thread
 * (CLSIMHIP_ERR_ARGUMENT / CLSIMHIP_ERR_CONFIG as above; CLSIMHIP_ERR_STATE with none of clsimhip_set_mcpe_series,
 * clsimhip_set_pmt_series, clsimhip_set_frame_photons and clsimhip_set_event_statistics).  A bunch enqueued with clsimhip_enqueue_steps has no table: one frame, 0. */
int clsimhip_enqueue_steps_with_particles(clsimhip_converter *c, const clsimhip_step *steps, size_t n, uint32_t identifier,
                                          const clsimhip_mcpe_particle *particles, size_t n_particles, const clsimhip_mcpe_mask *masked,
                                          size_t n_masked);
/* Records and series table of the result `photons` belongs to, valid until clsimhip_release_result(c, photons); n_masked (may be
 * NULL) receives the MASKED count.  Pointers are NULL where there is nothing.  CLSIMHIP_ERR_STATE without clsimhip_set_mcpe_series. */
int clsimhip_get_result_mcpe_series(clsimhip_converter *c, const clsimhip_photon *photons, const clsimhip_mcpe **mcpes, size_t *n,
                                    const clsimhip_mcpe_series **series, size_t *n_series, uint64_t *n_masked);

/* ---- MCPE merging: the records of a series within a time window become one, with the particle-ID map ----------------------
 * The reference never commits the unmerged series: I3CLSimClientModule pushes every MCPE through MCHitMerging::MCPEStream
 * (public/clsim/I3CLSimClientModule.h:193-194, private/clsim/I3CLSimClientModule.cxx:430) and at frame end puts
 * extractMCPEsWithPIDInfo()'s two objects into the frame (:710-719): the merged I3MCPESeriesMap (npe >= 1, the particle taken out
 * of the record) and <name>ParticleIDMap (per DOM and per particle, the indices of the merged MCPEs the particle contributed to);
 * the older module does the same behind its time sort (dom/I3PhotonToMCPEConverter.cxx:524-533).  The stream class lies outside
 * the reference (sim-services) and its result depends on insertion order, which no two runs repeat.  THE RULE BELOW IS THIS
 * PROJECT'S OWN DEFINITION, UNPINNED AGAINST THE REFERENCE; it exists once, compiled for the host twin and for the kernels.
 * Input: the output of the series stage -- records ascending in (frame, DOM rank, tkey, identifier), partitioned by the series
 * table.  Parameter: window, a binary64 with 0 <= window < +inf (anything else: CLSIMHIP_ERR_ARGUMENT; there is no default, the
 * reference's value lives outside the reference).  Per series, the records in order; a record OPENS A GROUP when
 *     it is the first record of its series, or
 *     its time is not finite, or
 *     the opener of the current group has a time that is not finite, or
 *     time - T > window, T the time of the record that opened the current group: one binary64 subtraction and one >, the rounded
 *     difference decides;
 * otherwise it joins the current group.  Groups never span series; particles do not matter for grouping.
 * One merged record per group: time = the opener's time, npe = the number of records in the group.  The merged series table has
 * the same entries in the same order as the input table; first and count refer to merged records.  The parent table is the
 * flattened I3ParticleIDMap: one entry per distinct (identifier, group) of a series, `index` = the group's position within its
 * series' merged records, ascending in (series, identifier, index); the parallel range table has one entry per series.
 * All outputs are functions of the input arrays: the same bytes from run to run, and from the kernels and the host twin.
 * fl(t - T) is monotone in t, so within the finite part of a series "the first record with t - T > window" is a well-defined
 * cut; the sum of npe is the number of input records; consecutive finite openers of a series differ by more than window; every
 * group spans at most window. */
typedef struct {
    uint32_t npe;
    int16_t string_id;
    uint16_t om_id;
    double time;
} clsimhip_mcpe_merged;                 /* 16 bytes */
typedef struct {
    uint32_t identifier;
    uint32_t index;                     /* of the merged record, within its series */
} clsimhip_mcpe_parent;                 /* 8 bytes */
typedef struct {
    uint32_t first, count;              /* parent entries [first, first + count) of one series */
} clsimhip_mcpe_parent_range;           /* 8 bytes */
typedef char clsimhip_mcpe_merged_is_16_bytes[sizeof(clsimhip_mcpe_merged) == 16 ? 1 : -1];
typedef char clsimhip_mcpe_parent_is_8_bytes[sizeof(clsimhip_mcpe_parent) == 8 ? 1 : -1];
typedef char clsimhip_mcpe_parent_range_is_8_bytes[sizeof(clsimhip_mcpe_parent_range) == 8 ? 1 : -1];
/* The host twin: a sequential walk, std::sort and std::unique for the parents.  Host only, no GPU is touched.  series must
 * partition the n records in order (CLSIMHIP_ERR_ARGUMENT otherwise).  out_merged and out_parents hold n entries each, out_series
 * and out_ranges n_series. */
int clsimhip_mcpe_merge_host(const clsimhip_mcpe *records, size_t n, const clsimhip_mcpe_series *series, size_t n_series, double window,
                             clsimhip_mcpe_merged *out_merged, clsimhip_mcpe_series *out_series, clsimhip_mcpe_parent *out_parents,
                             clsimhip_mcpe_parent_range *out_ranges, size_t *n_merged, size_t *n_parents);
/* bytes of device memory the kernels need beside their input and output, for up to `capacity` records */
size_t clsimhip_mcpe_merge_workspace_bytes(size_t capacity);
/* The kernels, on series that live in HBM (pairs with clsimhip_mcpe_series_device: d_records = its d_out, d_series and
 * d_series_counts = its d_series and d_counts): min(d_series_counts[0], capacity) records, min(d_series_counts[1], capacity)
 * series.  d_merged, d_merged_series, d_parents and d_ranges: `capacity` entries each, 8-byte aligned; d_counts: two uint32 --
 * merged records, parent entries; d_workspace: clsimhip_mcpe_merge_workspace_bytes(capacity) bytes, 16-byte aligned.
 * g: the generator whose series these are (it must be there; the stage itself needs nothing from it).  Asynchronous on hip_stream
 * (NULL = default stream); nothing waits for the device.  Errors are CLSIMHIP_ERR_ARGUMENT. */
int clsimhip_mcpe_merge_device(clsimhip_mcpe_generator *g, int device, const void *d_records, const void *d_series,
                               const void *d_series_counts, size_t capacity, double window, void *d_merged, void *d_merged_series,
                               void *d_parents, void *d_ranges, void *d_counts, void *d_workspace, size_t workspace_bytes, void *hip_stream);
/* The stage behind every bunch's series stage, on the bunch's stream.  Before Initialize() only (CLSIMHIP_ERR_STATE after);
 * Compile() refuses it without clsimhip_set_mcpe_series (CLSIMHIP_ERR_CONFIG).  on = 0 (the default): no launch, no byte changes
 * anywhere. */
int clsimhip_set_mcpe_merging(clsimhip_converter *c, int on, double window);
/* Merged records, merged series table, parent table and its ranges (n_series entries) of the result `photons` belongs to, valid
 * until clsimhip_release_result(c, photons); pointers are NULL where there is nothing.  clsimhip_get_result_mcpe_series keeps
 * returning the unmerged series of the same bunch.  CLSIMHIP_ERR_STATE without clsimhip_set_mcpe_merging. */
int clsimhip_get_result_mcpe_merged(clsimhip_converter *c, const clsimhip_photon *photons, const clsimhip_mcpe_merged **merged,
                                    size_t *n_merged, const clsimhip_mcpe_series **series, size_t *n_series,
                                    const clsimhip_mcpe_parent **parents, size_t *n_parents, const clsimhip_mcpe_parent_range **ranges);

/* ---- MCPE frame store: the series of several bunches accumulate per frame; finished frames leave ----------------------------
 * A frame's light is rarely one bunch.  The reference's client module files every result's hits into a frame cache that lives
 * across bunches (private/clsim/I3CLSimClientModule.cxx:359-439, frame->hits) and FlushFrameCache() commits a prefix of it, oldest
 * frames first, up to the last frame no bunch in flight still holds work for (:686-758, framesForBunches_, lastPendingFrame).  Here:
 * SERIES FORM: (records, table) as the series stage writes and the merging stage reads.  The table is strictly ascending in
 *     (frame, string_id signed, om_id); every count > 0; first[0] = 0 and first[s] = first[s-1] + count[s-1]; the last entry ends
 *     at the number of records (an empty table needs zero records); every record carries its entry's string_id and om_id; inside a
 *     series (tkey(time), identifier) does not descend.  Each element (entry or record) that breaks one of these rules is one
 *     MALFORMED element; the checks are local and together they imply the partition.
 * KEY of a record: (frame of its entry, string_id signed, om_id, tkey, identifier), compared as integers.
 * UNION(A, B): the series form of the multiset union -- records ascending in the key, the table rebuilt from the heads.  Ties take
 *     A's record first, which changes no byte.  Equal keys are equal bytes, so the union is a function of the multiset: the same
 *     bytes whatever order the bunches arrive in, and for any split of a bunch's MCPEs into two parts with one particle table and
 *     mask the union of their series is the series of the whole, byte for byte.  n_a + n_b must fit the output capacity.
 * SPLIT(X, last_frame): the head is the entries with frame <= last_frame and their records, a prefix; the tail is the rest with
 *     `first` rebased to 0.  last_frame = 0xFFFFFFFF drains everything.
 * The host twins (std::merge on the key; host only, no GPU is touched): malformed input or an output that does not fit is
 * CLSIMHIP_ERR_ARGUMENT with text that names the first offending element.  out_records and out_series hold out_capacity entries. */
int clsimhip_mcpe_series_union_host(const clsimhip_mcpe *a_records, size_t n_a, const clsimhip_mcpe_series *a_series, size_t n_series_a,
                                    const clsimhip_mcpe *b_records, size_t n_b, const clsimhip_mcpe_series *b_series, size_t n_series_b,
                                    clsimhip_mcpe *out_records, clsimhip_mcpe_series *out_series, size_t out_capacity, size_t *n, size_t *n_series);
int clsimhip_mcpe_series_split_host(const clsimhip_mcpe *records, size_t n, const clsimhip_mcpe_series *series, size_t n_series, uint32_t last_frame,
                                    clsimhip_mcpe *head_records, clsimhip_mcpe_series *head_series, size_t head_capacity, size_t *n_head,
                                    size_t *n_series_head, clsimhip_mcpe *tail_records, clsimhip_mcpe_series *tail_series, size_t tail_capacity,
                                    size_t *n_tail, size_t *n_series_tail);
/* bytes of device memory the union's kernels need beside their inputs and output */
size_t clsimhip_mcpe_series_union_workspace_bytes(size_t capacity_a, size_t capacity_b);
/* The kernels, on series that live in HBM.  Inputs are read as clsimhip_mcpe_merge_device reads them: min(counts[0], capacity)
 * records, min(counts[1], capacity) series.  d_out_records and d_out_series: out_capacity entries each; d_out_counts: five uint32
 * -- records, series, MALFORMED elements in A, MALFORMED elements in B, overflow (n_a + n_b when it does not fit out_capacity, else
 * 0); the first two follow the series stage's layout, so the output chains into another union, into the split and into
 * clsimhip_mcpe_merge_device unchanged.  When B is malformed or the union does not fit, the output is A unchanged (nothing, should
 * A alone not fit); when A is malformed, the output is empty.  Nothing is written beyond a capacity and every loop is bounded by
 * one, whatever bytes the inputs hold.  The output must not overlap an input.  Records, tables and d_workspace
 * (clsimhip_mcpe_series_union_workspace_bytes(capacity_a, capacity_b) bytes) are 16-byte aligned; capacities are at most 2^31.
 * Asynchronous on hip_stream (NULL = default stream); nothing waits for the device.  Errors are CLSIMHIP_ERR_ARGUMENT. */
int clsimhip_mcpe_series_union_device(int device, const void *d_a_records, const void *d_a_series, const void *d_a_counts, size_t capacity_a,
                                      const void *d_b_records, const void *d_b_series, const void *d_b_counts, size_t capacity_b,
                                      void *d_out_records, void *d_out_series, void *d_out_counts, size_t out_capacity, void *d_workspace,
                                      size_t workspace_bytes, void *hip_stream);
/* The split on the device; the input is taken as a series form and not checked again.  d_head_counts and d_tail_counts: five uint32
 * each in the union's layout -- records, series, 0, 0, overflow.  A head that does not fit head_capacity drains nothing: the head is
 * empty, the tail is everything, and the needed size goes into the head's overflow word.  tail_capacity >= capacity
 * (CLSIMHIP_ERR_ARGUMENT otherwise).  Asynchronous on hip_stream. */
int clsimhip_mcpe_series_split_device(int device, const void *d_records, const void *d_series, const void *d_counts, size_t capacity,
                                      uint32_t last_frame, void *d_head_records, void *d_head_series, void *d_head_counts, size_t head_capacity,
                                      void *d_tail_records, void *d_tail_series, void *d_tail_counts, size_t tail_capacity, void *hip_stream);
/* The store owns the accumulated series form and gives up finished frames.  device < 0: a host store, which uses only the twins and
 * needs no GPU.  A device store owns two record and table buffers of `capacity` entries, used in turn, its workspace, five sticky
 * counters and one event; every operation waits for the event on the caller's stream and records it again, so operations issued
 * on different streams are ordered as they were called.  capacity is at most 2^31. */
typedef struct clsimhip_mcpe_frame_store clsimhip_mcpe_frame_store;
int clsimhip_mcpe_frame_store_create(int device, size_t capacity, clsimhip_mcpe_frame_store **out);
void clsimhip_mcpe_frame_store_destroy(clsimhip_mcpe_frame_store *s);
const char *clsimhip_mcpe_frame_store_last_error(const clsimhip_mcpe_frame_store *s);
/* One bunch in host memory: validated on the host before anything moves (CLSIMHIP_ERR_ARGUMENT leaves the store unchanged; a host
 * store also refuses the bunch that does not fit).  A device store uploads it. */
int clsimhip_mcpe_frame_store_add_host(clsimhip_mcpe_frame_store *s, const clsimhip_mcpe *records, size_t n, const clsimhip_mcpe_series *series,
                                       size_t n_series);
/* One bunch in HBM (pairs with clsimhip_mcpe_series_device: its d_out, d_series and d_counts; capacity at most the store's).  Device
 * store only (CLSIMHIP_ERR_STATE otherwise), asynchronous on hip_stream.  A malformed bunch, or one that does not fit, is dropped
 * whole and counted in the sticky counters; the store carries on unchanged. */
int clsimhip_mcpe_frame_store_add_device(clsimhip_mcpe_frame_store *s, const void *d_records, const void *d_series, const void *d_series_counts,
                                         size_t capacity, void *hip_stream);
/* Moves the frames up to last_frame out on the device (for clsimhip_mcpe_merge_device behind it; d_counts: five uint32 as the
 * split's head); the tail becomes the store.  Device store only, asynchronous on hip_stream. */
int clsimhip_mcpe_frame_store_drain_device(clsimhip_mcpe_frame_store *s, uint32_t last_frame, void *d_records, void *d_series, void *d_counts,
                                           size_t capacity, void *hip_stream);
/* The same plus the download: the one call that waits.  With too small a capacity: CLSIMHIP_ERR_ARGUMENT, the store unchanged. */
int clsimhip_mcpe_frame_store_drain_host(clsimhip_mcpe_frame_store *s, uint32_t last_frame, clsimhip_mcpe *records, clsimhip_mcpe_series *series,
                                         size_t capacity, size_t *n, size_t *n_series);
/* What a drain up to last_frame would take.  Waits.  While any sticky counter is nonzero, both drain calls and this one return
 * CLSIMHIP_ERR_DEVICE with the counts in the text (a drain on the device learns of bunches whose union has run; its kernel looks
 * again) and nothing is delivered: data loss is loud, as a bunch with UNKNOWN_PARTICLE is. */
int clsimhip_mcpe_frame_store_size(clsimhip_mcpe_frame_store *s, uint32_t last_frame, size_t *n, size_t *n_series);

/* ---- Multi-PMT hit generator: detected photons -> hits on the PMTs of segmented modules ---------------------------------
 * The hit maker for modules that carry several PMTs (KM3NeT-style spheres): FindHitPMT and the per-photon body of
 * I3PhotonToMCHitConverterForMultiPMT::DAQ (private/clsim/dom/I3PhotonToMCHitConverterForMultiPMT.cxx:111-227, 297-382).  A pure
 * function of one delivered photon record (position relative to the module centre, string and OM IDs), a fixed configuration and
 * a 64-bit seed.  Per record, in this order:
 *     no module for the record's (string ID, OM ID) -> UNKNOWN_MODULE, no hit;
 *     direction d from the record's angles as the MCPE generator makes it; position . d > 0 (the photon is leaving) -> no hit;
 *     |position| not within 3 cm of the sphere radius of the module's type -> counted as OFF_SURFACE, and the record GOES ON (the
 *     reference only warns);
 *     every PMT of the type in index order, axis n and centre a rotated into the module's orientation: skipped when d . n >= 1e-8,
 *     when mu = ((a - position) . n) / (d . n) < 0, or when position + mu d is further from a than the PMT's radius; of several
 *     intersections the one with the smallest mu (a later one replaces an earlier one only if its mu is smaller); none -> no hit;
 *     c = -(n . d) <= 0 -> no hit (the reference's hit_angle >= 90 degrees, stated on the cosine);
 *     P = weight; P *= G_type(wavelength); P *= Q_pmt(wavelength) x collection efficiency; P *= A_pmt(c) / c;
 *     P > 1 -> PROBABILITY_ABOVE_ONE, no hit; a hit when P > u, u as for the MCPE generator (the record's hash and the seed);
 *     hit = {identifier, string ID, OM ID, PMT index within its type, time = the photon's time} (the reference computes a travel
 *     time inside the module and then stores the photon's own).
 * G (glass / gel survival), Q (quantum efficiency) and A (angular acceptance factor, tabulated over c = cos of the hit angle) are
 * clsimhip_functions of kinds TABLE and CONSTANT.  The path length the reference hands to the glass / gel survival is NOT modelled
 * (it needs an exponential the reference does not define).  Binary64 + - x / in one fixed order, as for the MCPE generator: the HIP
 * kernel and the host twin give the same bits, for every 80-byte pattern.  Angles of any size, infinite or NaN: as for the MCPE
 * generator.  Comparisons with a NaN are false, so a NaN direction skips no PMT and ends on the type's last one (a NaN path length is
 * replaced by any later intersection), and a NaN weight or P yields a hit.  The hit's time is the record's binary32 time widened:
 * infinities stay, a NaN keeps its sign and payload and is made quiet. */
typedef struct {
    double sphere_radius;               /* of the module's sphere [m]: the radius photons are recorded at */
    int32_t first_pmt, n_pmts;          /* its PMTs in the `pmts` array (1 ... 64); a hit's `pmt` counts from first_pmt */
    int32_t glass_gel_survival;         /* G: index into `functions`, over the wavelength */
    int32_t reserved;
} clsimhip_pmt_type;                    /* 24 bytes */
typedef struct {
    double axis[3];                     /* unit to 1e-6, module frame: the direction the PMT looks in */
    double position[3];                 /* centre of its disc [m], module frame; inside the sphere */
    double radius;                      /* of the disc [m] */
    double collection_efficiency;
    int32_t quantum_efficiency;         /* Q: index into `functions`, over the wavelength */
    int32_t angular_acceptance;         /* A: index into `functions`, over c */
} clsimhip_pmt;                         /* 72 bytes */
typedef struct {
    int32_t string_id;
    uint32_t om_id;
    int32_t type;                       /* index into `types` */
    int32_t reserved;
    double rotation[9];                 /* row-major, module frame -> detector frame (I3Orientation is outside the reference) */
} clsimhip_pmt_module;                  /* 88 bytes */
typedef struct {
    uint32_t identifier;                /* the photon's (I3MCHit::SetParticleID is the caller's, keyed by it) */
    int16_t string_id;
    uint16_t om_id;
    uint32_t pmt;                       /* PMT number within the module's type (the key of I3MCHitSeriesMultiOM) */
    uint32_t reserved;                  /* 0 */
    double time;
} clsimhip_pmt_hit;                     /* 24 bytes */
typedef char clsimhip_pmt_hit_is_24_bytes[sizeof(clsimhip_pmt_hit) == 24 ? 1 : -1];
typedef char clsimhip_pmt_is_72_bytes[sizeof(clsimhip_pmt) == 72 ? 1 : -1];
typedef char clsimhip_pmt_module_is_88_bytes[sizeof(clsimhip_pmt_module) == 88 ? 1 : -1];
#define CLSIMHIP_PMT_UNKNOWN_MODULE 0           /* index into the condition counters */
#define CLSIMHIP_PMT_PROBABILITY_ABOVE_ONE 1
#define CLSIMHIP_PMT_OFF_SURFACE 2
typedef struct clsimhip_pmt_generator clsimhip_pmt_generator;
/* At most 64 functions (3072 table values together), 8 types, 64 PMTs per type, 2^24 modules.  CLSIMHIP_ERR_CONFIG for: a limit
 * exceeded; a function of another kind than TABLE / CONSTANT; a rotation that changes the squared length of a unit vector (its
 * three columns, and every PMT axis and position of the module's type) by more than 1e-6; a PMT axis that is not unit to 1e-6; a
 * PMT whose position lies outside its type's sphere; a module whose type index names no type; a (string ID, OM ID) pair given
 * twice; IDs that do not fit the photon record.  Host only: no GPU is touched. */
int clsimhip_pmt_generator_create(const clsimhip_function *functions, size_t n_functions, const clsimhip_pmt_type *types, size_t n_types,
                                  const clsimhip_pmt *pmts, size_t n_pmts, const clsimhip_pmt_module *modules, size_t n_modules,
                                  uint64_t seed, clsimhip_pmt_generator **out);
/* a converter the generator was given to keeps it alive until the converter is destroyed */
void clsimhip_pmt_generator_destroy(clsimhip_pmt_generator *g);
const char *clsimhip_pmt_generator_last_error(const clsimhip_pmt_generator *g);
/* The host twin: the definition, for callers without a GPU and for the tests.  Keeps the input order.  *n_out = hits made (may
 * exceed `capacity`: only the first `capacity` are stored); counters[3] (may be NULL) receives the three condition counts. */
int clsimhip_pmt_convert_host(const clsimhip_pmt_generator *g, const clsimhip_photon *photons, size_t n, clsimhip_pmt_hit *out,
                              size_t capacity, size_t *n_out, uint64_t counters[3]);
/* The kernel, on records that live in HBM: min(*d_hit_count, capacity) records of d_photons (16-byte aligned).  d_hits: 8-byte
 * aligned.  d_counters: four uint32, zeroed by this call; [0] counts the hits and keeps counting past hit_capacity (only the first
 * hit_capacity are stored), [1] UNKNOWN_MODULE, [2] PROBABILITY_ABOVE_ONE, [3] OFF_SURFACE.  Output order is unspecified.
 * Asynchronous on hip_stream (NULL = default stream). */
int clsimhip_pmt_convert_device(clsimhip_pmt_generator *g, int device, const void *d_photons, const void *d_hit_count, size_t capacity,
                                void *d_hits, size_t hit_capacity, void *d_counters, void *hip_stream);
/* Attach the generator to a converter: the kernel then runs on every bunch's stream behind the propagation kernels, over the
 * records the bunch stored.  Before Initialize() only (CLSIMHIP_ERR_STATE after); g = NULL switches it off (the default: no launch
 * and no byte changes anywhere).  keep_photons as for clsimhip_set_mcpe_generator.  Compile() then refuses (CLSIMHIP_ERR_CONFIG):
 * an MCPE generator beside it; clsimhip_set_mcpe_series (the series of PMT hits are clsimhip_set_pmt_series'); a geometry DOM without a module or whose
 * IDs do not fit the record; a type in use whose sphere radius differs by more than 3 cm from the radius the converter records
 * photons at (the geometry's OM radius / the pancake factor); photon histories together with keep_photons = 0.
 * A bunch with UNKNOWN_MODULE or PROBABILITY_ABOVE_ONE > 0 fails as a bunch with one of the MCPE generator's conditions does, with
 * the counts in the text; OFF_SURFACE is reported on stderr and is not fatal. */
int clsimhip_set_pmt_generator(clsimhip_converter *c, clsimhip_pmt_generator *g, int keep_photons);
/* Hits of the result `photons` belongs to; valid until clsimhip_release_result(c, photons).  *hits is NULL when there are none. */
int clsimhip_get_result_pmt_hits(clsimhip_converter *c, const clsimhip_photon *photons, const clsimhip_pmt_hit **hits, size_t *n);

/* ---- PMT series: a bunch's PMT hits as per-frame, per-module, per-PMT time-sorted series ---------------------------------
 * What the reference does with every hit of a multi-PMT module on host threads: the client module files the photons under their
 * frames with the particles' time shifts and the frames' ignoreModules (private/clsim/I3CLSimClientModule.cxx:359-439), and
 * I3PhotonToMCHitConverterForMultiPMT::DAQ files every hit under its OMKey and then under its PMT number (I3MCHitSeriesMultiOMMap, a
 * map of maps) and time-sorts every PMT's vector (private/clsim/dom/I3PhotonToMCHitConverterForMultiPMT.cxx:291-292, 365, 387-395)
 * -- as a sorting stage behind the PMT hit kernel, the MCPE series' radix passes on a key of its own.
 * With the generator's modules ranked in ascending (string_id signed, om_id) order, base = the exclusive prefix sum of the modules'
 * PMT counts (the n_pmts of each module's type) in that order and n_channels its total, a hit's channel is base[module rank] + pmt.
 * Per record, in this order:
 *     its module is not one of the generator's, or pmt >= n_pmts of the module's type -> UNKNOWN_CHANNEL, no record (the
 *     generator's own hits never meet this);
 *     its identifier is not in the particle table -> UNKNOWN_PARTICLE, no record (log_fatal in the reference, :388-390); without a
 *     table the frame is 0 and the shift +0.0;
 *     (frame, string_id, om_id) is in the mask -> MASKED, no record (:399; not an error).  The mask is per module, as ignoreModules
 *     is: it masks all of the module's PMTs;
 *     time' = time + time_shift, one binary64 addition.
 * The kept records come out with reserved = 0, ascending in the 128-bit integer key (group = frame rank x n_channels + channel,
 * tkey(time'), identifier): frames in ascending frame ID, then modules, then PMTs, then the MCPE series' total order on the time's
 * bit pattern, then the identifier.  Records with equal keys are byte-identical, so the output is a function of the input as a
 * multiset: the same bytes from run to run and the same bytes from the kernels and the host twin.  The series table has one entry
 * per non-empty (frame, module, PMT) in the same order; its entries partition the records.
 * What differs from the reference, on purpose: its std::sort with < on doubles leaves the order of equal times and of NaNs
 * unspecified -- here the order is total on bit patterns, with the identifier as tie-break; it adds the shift to the photon's
 * binary32 time before the conversion -- here it is added once, to the hit's widened time, in binary64.  Not pinned against the
 * reference's output, like the rest of the multi-PMT hit maker (I3OMTypeInfo and I3Orientation are outside it).
 * The particle table and the mask are the MCPE series' (clsimhip_mcpe_particle, clsimhip_mcpe_mask), with the same checks. */
typedef struct {
    uint32_t frame;
    int16_t string_id;
    uint16_t om_id;
    uint32_t pmt;
    uint32_t first, count;              /* records [first, first + count) */
    uint32_t reserved;                  /* 0 */
} clsimhip_pmt_series;                  /* 24 bytes */
typedef char clsimhip_pmt_series_is_24_bytes[sizeof(clsimhip_pmt_series) == 24 ? 1 : -1];
#define CLSIMHIP_PMT_SERIES_UNKNOWN_PARTICLE 0  /* index into the series counters */
#define CLSIMHIP_PMT_SERIES_MASKED 1
#define CLSIMHIP_PMT_SERIES_UNKNOWN_CHANNEL 2
/* The host twin: the definition with std::sort on the key, for callers without a GPU and for the tests.  `g` supplies the modules
 * and their types.  particles = NULL, n_particles = 0: no table.  out and series hold n entries each; counters[3] (may be NULL)
 * receives the three counts.  CLSIMHIP_ERR_ARGUMENT for a table that is not strictly increasing in `identifier`,
 * CLSIMHIP_ERR_CONFIG when frames x n_channels >= 2^32. */
int clsimhip_pmt_series_host(const clsimhip_pmt_generator *g, const clsimhip_pmt_hit *hits, size_t n, const clsimhip_mcpe_particle *particles,
                             size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked, clsimhip_pmt_hit *out,
                             clsimhip_pmt_series *series, size_t *n_kept, size_t *n_series, uint64_t counters[3]);
/* bytes of device memory the kernels need beside their input and output, for up to `capacity` records and a bunch with this table
 * and mask */
size_t clsimhip_pmt_series_workspace_bytes(size_t capacity, size_t n_particles, size_t n_masked);
/* The kernels, on hits that live in HBM (pairs with clsimhip_pmt_convert_device: d_hits and d_count = its d_counters, whose first
 * word counts past the capacity): min(*d_count, capacity) records of d_hits.  d_out and d_series: `capacity` entries each, 8-byte
 * aligned; d_workspace: clsimhip_pmt_series_workspace_bytes(capacity, n_particles, n_masked) bytes, 16-byte aligned; d_counts: five
 * uint32 -- records kept, series, then the three counters (CLSIMHIP_ERR_ARGUMENT for a misaligned pointer or a workspace that is
 * too small; nothing is launched then).  The particle table and the mask are host memory: they are checked and copied before the
 * call returns (which may wait for the previous call's copy, nothing else); the kernels are asynchronous on hip_stream (NULL =
 * default stream) and nothing else waits for the device. */
int clsimhip_pmt_series_device(clsimhip_pmt_generator *g, int device, const void *d_hits, const void *d_count, size_t capacity,
                               const clsimhip_mcpe_particle *particles, size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked,
                               void *d_out, void *d_series, void *d_counts, void *d_workspace, size_t workspace_bytes, void *hip_stream);
/* The stage behind every bunch's PMT hit kernel, on the bunch's stream.  Before Initialize() only (CLSIMHIP_ERR_STATE after);
 * Compile() refuses it without a PMT hit generator (CLSIMHIP_ERR_CONFIG, "need a PMT hit generator").  on = 0 (the default): no
 * launch and no byte changes anywhere.  With it on, clsimhip_enqueue_steps_with_particles takes the bunch's table and mask,
 * clsimhip_get_result_pmt_hits returns the sorted records, and a bunch with UNKNOWN_PARTICLE or UNKNOWN_CHANNEL > 0 fails as a bunch
 * with one of the generator's conditions does (CLSIMHIP_ERR_DEVICE, the counts in the text). */
int clsimhip_set_pmt_series(clsimhip_converter *c, int on);
/* Sorted hits and series table of the result `photons` belongs to, valid until clsimhip_release_result(c, photons); n_masked (may
 * be NULL) receives the MASKED count.  Pointers are NULL where there is nothing.  CLSIMHIP_ERR_STATE without clsimhip_set_pmt_series. */
int clsimhip_get_result_pmt_series(clsimhip_converter *c, const clsimhip_photon *photons, const clsimhip_pmt_hit **hits, size_t *n,
                                   const clsimhip_pmt_series **series, size_t *n_series, uint64_t *n_masked);

/* ---- Frame photons: a bunch's detected photons as per-frame, per-module sorted series -------------------------------------
 * The client module's default output, PhotonSeriesMapName = "PropagatedPhotons": an I3CompressedPhotonSeriesMap that
 * AddPhotonsToFrames (private/clsim/I3CLSimClientModule.cxx:359-439) builds at :407-415 through Emit<I3CompressedPhoton>
 * (:327-349) -- as a sorting stage behind the propagation kernel's photon records, the MCPE series' radix passes run twice.
 * ("Frame photons", because clsimhip_photon_series_* is the wire format above.)  Per clsimhip_photon, in this order:
 *     its module is not in the stage's DOM list -> UNKNOWN_DOM, no record;
 *     its identifier is not in the particle table -> UNKNOWN_PARTICLE, no record (log_fatal in the reference, :388-390); without a
 *     table the frame is 0 and the shift +0.0;
 *     (frame, string_id, om_id) is in the mask -> MASKED, no record (:399; not an error);
 *     time' = (double)time + time_shift, one binary64 addition (:334), which quiets a signalling NaN; weight, wavelength,
 *     group_velocity, x, y, z, theta and phi are copied bit for bit.  theta and phi stay as the propagator stored them: the
 *     reference passes them through I3Direction::SetThetaPhi, which lies outside it.
 * The kept records come out ascending in
 *     frame (ascending frame ID), module (ascending (string_id signed, om_id): OMKey::operator<), tkey(time'), identifier, h,
 *     w0 ... w7
 * where tkey is the MCPE series' total order on the time's bit pattern, w0 ... w7 are the eight float fields as uint32 bit patterns
 * in declared order, and h is FNV-1a over their 32 bytes: h = 2166136261; for each word w0 ... w7, for each of its bytes from the least
 * significant one: h = (h ^ byte) * 16777619 (mod 2^32).  h decides order, so it is part of this contract.  Records equal in all of
 * that are byte-identical, so the output is a function of the input as a multiset: the same bytes from run to run, whatever the
 * schedule, and the same bytes from the kernels and the host twin.  The series table (clsimhip_mcpe_series: frame, module, first,
 * count) has one entry per non-empty (frame, module) in the same order; its entries partition the records.
 * What differs from the reference, on purpose: it appends to each (frame, ModuleKey) vector in arrival order, which no two runs
 * repeat -- here the order within a series is the one above; it adds the shift in the photon's binary32 -- here once, in binary64.
 * One bound keeps every input's cost bounded.  Take a run of records equal in (frame, module, tkey, identifier, h) that holds at
 * least two distinct contents: if it has more than 2 048 members, each member is counted as TIE_OVERFLOW and the call delivers no
 * records (kept = series = 0); a bunch behind the converter fails then, as it does for UNKNOWN_PARTICLE.  A run of identical records
 * of any length is fine.  Reaching the bound takes crafted 32-bit collisions at one module, time and particle. */
typedef struct {
    uint32_t identifier;
    int16_t string_id;
    uint16_t om_id;
    double time;
    float weight, wavelength, group_velocity, x, y, z, theta, phi;
} clsimhip_frame_photon;                /* 48 bytes */
typedef char clsimhip_frame_photon_is_48_bytes[sizeof(clsimhip_frame_photon) == 48 ? 1 : -1];
#define CLSIMHIP_FRAME_PHOTONS_UNKNOWN_PARTICLE 0       /* index into the four counters */
#define CLSIMHIP_FRAME_PHOTONS_MASKED 1
#define CLSIMHIP_FRAME_PHOTONS_UNKNOWN_DOM 2
#define CLSIMHIP_FRAME_PHOTONS_TIE_OVERFLOW 3
#define CLSIMHIP_FRAME_PHOTONS_TIE_BOUND 2048
/* The stage's DOM list (host only): the modules a photon may be filed under.  A pair named twice is one DOM.
 * CLSIMHIP_ERR_ARGUMENT for a string ID outside int16 or an OM ID outside uint16. */
typedef struct clsimhip_frame_photon_doms clsimhip_frame_photon_doms;
int clsimhip_frame_photon_doms_create(size_t n_doms, const int32_t *string_ids, const uint32_t *om_ids, clsimhip_frame_photon_doms **out);
void clsimhip_frame_photon_doms_destroy(clsimhip_frame_photon_doms *d);
const char *clsimhip_frame_photon_doms_last_error(const clsimhip_frame_photon_doms *d);
/* The host twin: the definition with std::sort on the full order, for callers without a GPU and for the tests.  particles = NULL,
 * n_particles = 0: no table.  out and series hold n entries each; counters[4] (may be NULL) receives the four counts.
 * CLSIMHIP_ERR_ARGUMENT for a table that is not strictly increasing in `identifier`, CLSIMHIP_ERR_CONFIG when frames x DOMs >= 2^32. */
int clsimhip_frame_photons_host(const clsimhip_frame_photon_doms *d, const clsimhip_photon *photons, size_t n, const clsimhip_mcpe_particle *particles,
                                size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked, clsimhip_frame_photon *out,
                                clsimhip_mcpe_series *series, size_t *n_kept, size_t *n_series, uint64_t counters[4]);
/* bytes of device memory the kernels need beside their input and output, for up to `capacity` records and a bunch with this table
 * and mask */
size_t clsimhip_frame_photons_workspace_bytes(size_t capacity, size_t n_particles, size_t n_masked);
/* The kernels, on photon records that live in HBM with string and OM IDs in them: min(*d_count, capacity) records of d_photons.
 * d_out and d_series: `capacity` entries each; d_photons, d_out, d_series and d_workspace
 * (clsimhip_frame_photons_workspace_bytes(capacity, n_particles, n_masked) bytes) 16-byte aligned; d_counts: six uint32 -- records
 * kept, series, then the four counters (CLSIMHIP_ERR_ARGUMENT for a misaligned pointer or a workspace that is too small; nothing is
 * launched then).  The particle table and the mask are host memory: they are checked and copied before the call returns (which may
 * wait for the previous call's copy, nothing else); the kernels are asynchronous on hip_stream (NULL = default stream) and nothing
 * else waits for the device. */
int clsimhip_frame_photons_device(clsimhip_frame_photon_doms *d, int device, const void *d_photons, const void *d_count, size_t capacity,
                                  const clsimhip_mcpe_particle *particles, size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked,
                                  void *d_out, void *d_series, void *d_counts, void *d_workspace, size_t workspace_bytes, void *hip_stream);
/* The stage behind every bunch's propagation kernel, on the bunch's stream, with the geometry's DOMs as its list; independent of the
 * hit generators and of their series stages, beside which it may run.  Before Initialize() only (CLSIMHIP_ERR_STATE after).
 * on = 0 (the default): no launch, no allocation, no byte changes anywhere.  keep_photons = 0: the 80-byte records do not cross to
 * the host, and the result's `photons` pointer is only the handle, as for the MCPE generator (Compile() refuses photon histories
 * then, and a geometry whose IDs do not fit the record: CLSIMHIP_ERR_CONFIG).  With it on,
 * clsimhip_enqueue_steps_with_particles takes the bunch's table and mask, and a bunch with UNKNOWN_PARTICLE, UNKNOWN_DOM or
 * TIE_OVERFLOW > 0 fails (CLSIMHIP_ERR_DEVICE, the counts in the text). */
int clsimhip_set_frame_photons(clsimhip_converter *c, int on, int keep_photons);
/* Records and series table of the result `photons` belongs to, valid until clsimhip_release_result(c, photons); n_masked (may be
 * NULL) receives the MASKED count.  Pointers are NULL where there is nothing.  CLSIMHIP_ERR_STATE without clsimhip_set_frame_photons. */
int clsimhip_get_result_frame_photons(clsimhip_converter *c, const clsimhip_photon *photons, const clsimhip_frame_photon **records, size_t *n,
                                      const clsimhip_mcpe_series **series, size_t *n_series, uint64_t *n_masked);

/* ---- Frame photon store: the frame photons of several bunches accumulate per frame; finished frames leave --------------------
 * Frame photons, continued: what the MCPE frame store is for MCPEs, for clsimhip_frame_photon records with their clsimhip_mcpe_series
 * table -- the reference files every result's photons into (*frame->photons)[ModuleKey] of a frame cache that lives across bunches
 * (private/clsim/I3CLSimClientModule.cxx:359-439, :407-415) and FlushFrameCache() commits the oldest frames (:686-758).
 * SERIES FORM OF FRAME PHOTONS: the table rules are the MCPE frame store's; every record carries its entry's string_id and
 *     om_id; inside a series the 12-word suffix (tkey(time) high, low, identifier, h, w0 ... w7) does not descend, h and w as the
 *     frame photons stage defines them.  Each element (entry or record) that breaks a rule is one MALFORMED element.
 * KEY of a record: 14 words -- frame of its entry, module (string_id signed, om_id), tkey high, tkey low, identifier, h, w0 ... w7 --
 *     compared word by word as unsigned integers.  Equal keys are equal bytes.  The time travels as its bit pattern (tkey is an
 *     inversion on the bits), so a signalling NaN keeps its payload.
 * UNION(A, B): the multiset union ascending in the key, ties A first, the table rebuilt from the heads.  The comparison is the full
 *     key, so there is NO TIE BOUND: a run equal in (frame, module, tkey, identifier, h) of any length and any contents is ordered,
 *     also where the frame photons stage on the whole bunch would report TIE_OVERFLOW.  For any split of a bunch's photons into two
 *     parts with one particle table and mask, the union of their frame photons is the frame photons of the whole, byte for byte,
 *     wherever the whole has TIE_OVERFLOW = 0.
 * SPLIT(X, last_frame): the head is the entries with frame <= last_frame and their records; the tail is the rest, rebased.
 * Failure rules, the five output counts (records, series, MALFORMED elements in A, in B, overflow), capacities, alignment and
 * asynchrony are the MCPE frame store's, call for call: B malformed or an output that does not fit -> the output is A unchanged; A
 * malformed -> the output is empty; a head that does not fit drains nothing.  The counts keep (records, series) first, so a union's
 * output or a drain chains unchanged into clsimhip_photon_hits_device, clsimhip_pmt_photon_hits_device and another union. */
int clsimhip_frame_photons_union_host(const clsimhip_frame_photon *a_records, size_t n_a, const clsimhip_mcpe_series *a_series, size_t n_series_a,
                                      const clsimhip_frame_photon *b_records, size_t n_b, const clsimhip_mcpe_series *b_series, size_t n_series_b,
                                      clsimhip_frame_photon *out_records, clsimhip_mcpe_series *out_series, size_t out_capacity, size_t *n, size_t *n_series);
int clsimhip_frame_photons_split_host(const clsimhip_frame_photon *records, size_t n, const clsimhip_mcpe_series *series, size_t n_series, uint32_t last_frame,
                                      clsimhip_frame_photon *head_records, clsimhip_mcpe_series *head_series, size_t head_capacity, size_t *n_head,
                                      size_t *n_series_head, clsimhip_frame_photon *tail_records, clsimhip_mcpe_series *tail_series, size_t tail_capacity,
                                      size_t *n_tail, size_t *n_series_tail);
size_t clsimhip_frame_photons_union_workspace_bytes(size_t capacity_a, size_t capacity_b);
int clsimhip_frame_photons_union_device(int device, const void *d_a_records, const void *d_a_series, const void *d_a_counts, size_t capacity_a,
                                        const void *d_b_records, const void *d_b_series, const void *d_b_counts, size_t capacity_b,
                                        void *d_out_records, void *d_out_series, void *d_out_counts, size_t out_capacity, void *d_workspace,
                                        size_t workspace_bytes, void *hip_stream);
int clsimhip_frame_photons_split_device(int device, const void *d_records, const void *d_series, const void *d_counts, size_t capacity,
                                        uint32_t last_frame, void *d_head_records, void *d_head_series, void *d_head_counts, size_t head_capacity,
                                        void *d_tail_records, void *d_tail_series, void *d_tail_counts, size_t tail_capacity, void *hip_stream);
/* The store, as clsimhip_mcpe_frame_store: device < 0 is a host store on the twins; a device store owns two record and two table
 * buffers used in turn, a workspace, five sticky counters in page-locked memory and one event that every operation waits for and
 * records again.  add_device pairs with clsimhip_frame_photons_device (its d_out, d_series, d_counts).  A bunch dropped on the
 * device makes every later drain and _size return CLSIMHIP_ERR_DEVICE with the counts in the text -- once the host can see it:
 * _size and drain_host wait for the store's event first and always see it; drain_device does not wait, so while the add_device that
 * drops the bunch is still in flight it returns CLSIMHIP_OK, its kernel looks at the counters again on the device and delivers an
 * EMPTY head (records = series = 0 in d_counts, the store unchanged), and the error is raised by the next call that waits. */
typedef struct clsimhip_frame_photon_store clsimhip_frame_photon_store;
int clsimhip_frame_photon_store_create(int device, size_t capacity, clsimhip_frame_photon_store **out);
void clsimhip_frame_photon_store_destroy(clsimhip_frame_photon_store *s);
const char *clsimhip_frame_photon_store_last_error(const clsimhip_frame_photon_store *s);
int clsimhip_frame_photon_store_add_host(clsimhip_frame_photon_store *s, const clsimhip_frame_photon *records, size_t n, const clsimhip_mcpe_series *series,
                                         size_t n_series);
int clsimhip_frame_photon_store_add_device(clsimhip_frame_photon_store *s, const void *d_records, const void *d_series, const void *d_series_counts,
                                           size_t capacity, void *hip_stream);
int clsimhip_frame_photon_store_drain_device(clsimhip_frame_photon_store *s, uint32_t last_frame, void *d_records, void *d_series, void *d_counts,
                                             size_t capacity, void *hip_stream);
int clsimhip_frame_photon_store_drain_host(clsimhip_frame_photon_store *s, uint32_t last_frame, clsimhip_frame_photon *records, clsimhip_mcpe_series *series,
                                           size_t capacity, size_t *n, size_t *n_series);
int clsimhip_frame_photon_store_size(clsimhip_frame_photon_store *s, uint32_t last_frame, size_t *n, size_t *n_series);

/* ---- PMT hit frame store: the PMT hit series of several bunches accumulate per frame; finished frames leave --------------------
 * PMT series, continued: what the MCPE frame store is for MCPEs and the frame photon store for frame photons, for clsimhip_pmt_hit
 * records with their clsimhip_pmt_series table -- the reference files every result into a frame cache that lives across bunches
 * (private/clsim/I3CLSimClientModule.cxx:359-439) and FlushFrameCache() commits the oldest frames no bunch in flight can still
 * touch (:686-758).  With keep_photons = 0 there are no frame photons to accumulate, and this store is what joins bunches.
 * SERIES FORM OF PMT HITS: (records, table) as clsimhip_pmt_series_device and clsimhip_pmt_photon_hits_device write them.  The
 *     table is strictly ascending in (frame, string_id signed, om_id, pmt); every count > 0; first[0] = 0 and first[s] =
 *     first[s-1] + count[s-1]; the last entry ends at the number of records (an empty table needs zero records); every entry has
 *     reserved == 0; every record carries its entry's string_id, om_id and pmt and has reserved == 0; inside a series
 *     (tkey(time), identifier) does not descend.  Each element (entry or record) that breaks one of these rules is one MALFORMED
 *     element.  The checks are local -- an entry looks at itself and its predecessor, a record at its entry and its predecessor --
 *     and together they imply the partition and the global order.  The two reserved rules are what make equal keys equal bytes.
 * KEY of a record: six 32-bit words, most significant first -- frame of its entry, module (string_id signed, om_id), pmt (the
 *     whole word, not only values below 64), tkey high, tkey low, identifier -- compared as unsigned integers.  The time travels as
 *     its bit pattern (tkey is an inversion on the bits; no floating-point value is formed), so a signalling NaN keeps its payload:
 *     negative NaNs come first, then -inf ... -0, +0 ... +inf, positive NaNs last.
 * UNION(A, B): the series form of the multiset union, ties A first, which changes no byte, the table rebuilt from the heads.  Equal
 *     keys are equal bytes, so the union is a function of the multiset: the same bytes whatever order the bunches arrive in, and
 *     for any split of a bunch's hits into two parts with one particle table and mask the union of their PMT series is the PMT
 *     series of the whole, byte for byte.  n_a + n_b must fit the output capacity.
 * SPLIT(X, last_frame): the head is the entries with frame <= last_frame and their records, a prefix; the tail is the rest with
 *     `first` rebased to 0.  last_frame = 0xFFFFFFFF drains everything.
 * The host twins (std::merge on the key; host only, no GPU is touched): malformed input or an output that does not fit is
 * CLSIMHIP_ERR_ARGUMENT with text that names the first offending element. */
int clsimhip_pmt_hits_union_host(const clsimhip_pmt_hit *a_records, size_t n_a, const clsimhip_pmt_series *a_series, size_t n_series_a,
                                 const clsimhip_pmt_hit *b_records, size_t n_b, const clsimhip_pmt_series *b_series, size_t n_series_b,
                                 clsimhip_pmt_hit *out_records, clsimhip_pmt_series *out_series, size_t out_capacity, size_t *n, size_t *n_series);
int clsimhip_pmt_hits_split_host(const clsimhip_pmt_hit *records, size_t n, const clsimhip_pmt_series *series, size_t n_series, uint32_t last_frame,
                                 clsimhip_pmt_hit *head_records, clsimhip_pmt_series *head_series, size_t head_capacity, size_t *n_head,
                                 size_t *n_series_head, clsimhip_pmt_hit *tail_records, clsimhip_pmt_series *tail_series, size_t tail_capacity,
                                 size_t *n_tail, size_t *n_series_tail);
/* bytes of device memory the union's kernels need beside their inputs and output */
size_t clsimhip_pmt_hits_union_workspace_bytes(size_t capacity_a, size_t capacity_b);
/* The kernels, on series that live in HBM.  Inputs are read as min(counts[0], capacity) records and min(counts[1], capacity) series,
 * so clsimhip_pmt_series_device's five-word d_counts and clsimhip_pmt_photon_hits_device's seven-word d_counts chain in unchanged.
 * d_out_counts: five uint32 -- records, series, MALFORMED elements in A, MALFORMED elements in B, overflow (n_a + n_b when it does
 * not fit out_capacity, else 0).  When B is malformed or the union does not fit, the output is A unchanged (nothing, should A alone
 * not fit); when A is malformed, the output is empty.  Nothing is written beyond a capacity and every loop is bounded by one,
 * whatever bytes the inputs hold.  The output must not overlap an input.  Records and tables are 8-byte aligned (what
 * clsimhip_pmt_series_device produces; 24-byte elements cannot promise more), d_workspace
 * (clsimhip_pmt_hits_union_workspace_bytes(capacity_a, capacity_b) bytes) 16-byte aligned; capacities are at most 2^31.
 * Asynchronous on hip_stream (NULL = default stream); nothing waits for the device.  Errors are CLSIMHIP_ERR_ARGUMENT, with nothing
 * launched. */
int clsimhip_pmt_hits_union_device(int device, const void *d_a_records, const void *d_a_series, const void *d_a_counts, size_t capacity_a,
                                   const void *d_b_records, const void *d_b_series, const void *d_b_counts, size_t capacity_b,
                                   void *d_out_records, void *d_out_series, void *d_out_counts, size_t out_capacity, void *d_workspace,
                                   size_t workspace_bytes, void *hip_stream);
/* The split on the device; the input is taken as a series form and not checked again.  d_head_counts and d_tail_counts: five uint32
 * each -- records, series, 0, 0, overflow.  A head that does not fit head_capacity drains nothing: the head is empty, the tail is
 * everything, and the needed size goes into the head's overflow word.  tail_capacity >= capacity (CLSIMHIP_ERR_ARGUMENT otherwise). */
int clsimhip_pmt_hits_split_device(int device, const void *d_records, const void *d_series, const void *d_counts, size_t capacity,
                                   uint32_t last_frame, void *d_head_records, void *d_head_series, void *d_head_counts, size_t head_capacity,
                                   void *d_tail_records, void *d_tail_series, void *d_tail_counts, size_t tail_capacity, void *hip_stream);
/* The store, as clsimhip_mcpe_frame_store: device < 0 is a host store on the twins that touches no GPU; a device store owns two
 * record and two table buffers used in turn, a workspace, five sticky counters in page-locked memory and one event that every
 * operation waits for and records again, so operations issued on different streams are ordered as they were called.  add_host
 * validates the bunch on the host before anything moves; add_device pairs with clsimhip_pmt_series_device and
 * clsimhip_pmt_photon_hits_device (their d_out, d_series, d_counts) and refuses at once a bunch buffer longer than the store's
 * capacity.  A bunch dropped on the device (malformed, or one that does not fit) is counted in the sticky counters; while one is
 * nonzero, _size and both drains return CLSIMHIP_ERR_DEVICE with the counts in the text and nothing is delivered.  _size and
 * drain_host wait for the store's event first and always see it; drain_device does not wait, so while the add_device that drops the
 * bunch is still in flight it returns CLSIMHIP_OK, its kernel looks at the counters again on the device and delivers an EMPTY head,
 * and the error is raised by the next call that waits. */
typedef struct clsimhip_pmt_hit_store clsimhip_pmt_hit_store;
int clsimhip_pmt_hit_store_create(int device, size_t capacity, clsimhip_pmt_hit_store **out);
void clsimhip_pmt_hit_store_destroy(clsimhip_pmt_hit_store *s);
const char *clsimhip_pmt_hit_store_last_error(const clsimhip_pmt_hit_store *s);
int clsimhip_pmt_hit_store_add_host(clsimhip_pmt_hit_store *s, const clsimhip_pmt_hit *records, size_t n, const clsimhip_pmt_series *series, size_t n_series);
int clsimhip_pmt_hit_store_add_device(clsimhip_pmt_hit_store *s, const void *d_records, const void *d_series, const void *d_series_counts, size_t capacity,
                                      void *hip_stream);
int clsimhip_pmt_hit_store_drain_device(clsimhip_pmt_hit_store *s, uint32_t last_frame, void *d_records, void *d_series, void *d_counts, size_t capacity,
                                        void *hip_stream);
int clsimhip_pmt_hit_store_drain_host(clsimhip_pmt_hit_store *s, uint32_t last_frame, clsimhip_pmt_hit *records, clsimhip_pmt_series *series, size_t capacity,
                                      size_t *n, size_t *n_series);
int clsimhip_pmt_hit_store_size(clsimhip_pmt_hit_store *s, uint32_t last_frame, size_t *n, size_t *n_series);

/* ---- Cable shadow: drop detected photons whose last path crosses a cable ------------------------------------------------------
 * The reference's I3ShadowedPhotonRemoverModule (private/clsim/shadow/): PropagatedPhotons -> PropagatedPhotonsWithShadow, which its
 * photon-to-MCPE converter then reads.  I3ShadowedPhotonRemover::IsPhotonShadowed (I3ShadowedPhotonRemover.cxx:63-81) walks the
 * whole I3CylinderMap -- one cylinder per DOM from python/shadow/AddCylinder.py:38-65 -- for every photon on one host thread; here
 * that is a stage behind the propagation kernel.  Two things there cannot be restated, so the rule is this library's own: the
 * cylinder test it calls (I3ExtraGeometryItemCylinder::DoesLineIntersect) lies outside the reference, and its start point computes
 * dy with cos(azimuth) (:68; "This code is NOT functional at the moment").  The rule uses the corrected y component.
 * Arithmetic: binary64 + - * / in the order written, never contracted, no sqrt, no fma; mcpe_sincos is the deterministic
 * single-precision sine and cosine the hit makers use, its results widened.  It decides booleans only.
 * Per record, with `distance` D (finite, >= 0):
 *     P1 = ((double)x, (double)y, (double)z)
 *     (st, ct) = mcpe_sincos(theta)
 *     (sp, cp) = mcpe_sincos(phi)
 *     dir = ((double)st*(double)cp, (double)st*(double)sp, (double)ct)
 *     d   = D*dir
 *     P0  = P1 - d
 * P0 is the point D back along the arrival direction.  The reference's zenith and azimuth are those of -dir.
 * Per cylinder, precomputed once on the host, in this order:
 *     A  = bottom
 *     a  = top - bottom
 *     L2 = a.a
 *     r2 = r*r
 * Then, with m = P0 - A, and dot products taken as x*x' + y*y' + z*z' left to right:
 *     ma = m.a;  da = d.a;  u1 = ma + da
 *     if (ma < 0 && u1 < 0) || (ma > L2 && u1 > L2)  -> miss            (both ends beyond the same cap)
 *     lo = 0; hi = 1
 *     if da != 0:
 *         ta = (0 - ma)/da;  tb = (L2 - ma)/da
 *         if ta > tb: swap
 *         if ta > lo: lo = ta
 *         if tb < hi: hi = tb
 *         if lo > hi: miss
 *     else if !(ma >= 0 && ma <= L2): miss
 *     dd = d.d;  mm = m.m;  md = m.d
 *     al = dd*L2 - da*da;  be = md*L2 - ma*da;  ga = (mm - r2)*L2 - ma*ma
 *     t = lo
 *     if al > 0:
 *         t = (0 - be)/al;  if t < lo: t = lo;  if t > hi: t = hi
 *     hit  <=>  (al*t + (be + be))*t + ga <= 0
 * This is "the segment meets the solid finite cylinder".  The radial condition is a convex quadratic in t.  Its minimum over the
 * slab interval clipped to [0, 1] sits at the clamped vertex.
 * A record is shadowed iff some cylinder hits.  The set's order cannot matter.
 *   - A NaN in position or angles is never shadowed, because every comparison is false.
 *   - D = 0 is a point-in-cylinder test.
 *   - The position is used as stored.  With oversized DOMs it lies on the oversized sphere, and what that means is the caller's
 *     business.
 * The lit (not shadowed) records keep their input order, so the kernels and the host twin compare as arrays. */
#define CLSIMHIP_CABLE_SHADOW_MAX_CYLINDERS 16384
/* The cylinder set (host only): n_cylinders cylinders, top and bottom 3 doubles each, radius one.  CLSIMHIP_ERR_ARGUMENT for a
 * non-finite value, a radius <= 0, a cylinder whose L2 is zero or not finite, a distance that is negative or not finite,
 * n_cylinders = 0 and n_cylinders > CLSIMHIP_CABLE_SHADOW_MAX_CYLINDERS (which bounds the work of a launch at capacity x 16 384
 * tests). */
typedef struct clsimhip_cable_shadow clsimhip_cable_shadow;
int clsimhip_cable_shadow_create(size_t n_cylinders, const double *top, const double *bottom, const double *radius, double distance,
                                 clsimhip_cable_shadow **out);
void clsimhip_cable_shadow_destroy(clsimhip_cable_shadow *s);
const char *clsimhip_cable_shadow_last_error(const clsimhip_cable_shadow *s);
/* The host twin: flags holds n bytes (1 = shadowed), lit n records (the records with flag 0, in input order; *n_lit of them);
 * counts (may be NULL) receives records tested and records shadowed. */
int clsimhip_cable_shadow_host(const clsimhip_cable_shadow *s, const clsimhip_photon *photons, size_t n, uint8_t *flags, clsimhip_photon *lit,
                               size_t *n_lit, uint64_t counts[2]);
/* bytes of device memory the kernels need beside their input and output, for up to `capacity` records */
size_t clsimhip_cable_shadow_workspace_bytes(size_t capacity);
/* The kernels, on photon records that live in HBM: min(*d_count, capacity) records of d_photons.  d_flags: `capacity` bytes, of
 * which the first min(*d_count, capacity) are written; d_lit: `capacity` records; d_photons, d_lit and d_workspace
 * (clsimhip_cable_shadow_workspace_bytes(capacity) bytes) 16-byte aligned; d_counts: three uint32 -- records lit, tested, shadowed
 * (CLSIMHIP_ERR_ARGUMENT for a misaligned pointer or a workspace that is too small; nothing is launched then).  (d_lit, d_counts)
 * pair with every *_device call above as (d_photons, d_count) do.  The kernels are asynchronous on hip_stream (NULL = default
 * stream); the first call on a device copies the cylinder table there, nothing else waits for the device. */
int clsimhip_cable_shadow_device(clsimhip_cable_shadow *s, int device, const void *d_photons, const void *d_count, size_t capacity, void *d_flags,
                                 void *d_lit, void *d_counts, void *d_workspace, size_t workspace_bytes, void *hip_stream);
/* The stage right behind every bunch's propagation kernel, on the bunch's stream (s = NULL: off, the default -- no launch, no
 * allocation, no byte changes anywhere).  Before Initialize() only (CLSIMHIP_ERR_STATE after).  With it on, the MCPE generator with
 * its series and merging, the PMT hit generator with its series and the frame photons stage read the lit records where they read the
 * detected ones.  The 80-byte photons a result carries stay ALL detected photons -- the propagator's result, and the RNG states are
 * untouched; the reference keeps both maps too.  The set is fixed at Initialize(), like the geometry; the object may be destroyed
 * once this call has returned. */
int clsimhip_set_cable_shadow(clsimhip_converter *c, clsimhip_cable_shadow *s);
/* Flags of the result `photons` belongs to, aligned with its photon records (1 = shadowed; *n = the records the result carries, 0
 * with them NULL when the records did not cross to the host), and counts: records tested and shadowed, always delivered.  Valid
 * until clsimhip_release_result(c, photons).  CLSIMHIP_ERR_STATE without clsimhip_set_cable_shadow. */
int clsimhip_get_result_cable_shadow(clsimhip_converter *c, const clsimhip_photon *photons, const uint8_t **flags, size_t *n, uint64_t counts[2]);

/* ---- Event statistics: per particle, photons generated and photons at DOMs as counts and exact weight sums ------------------
 * The reference's I3CLSimEventStatistics (the client module's StatisticsName): per particle a count and a weight sum of the photons
 * generated, accumulated over the steps as they are enqueued (private/clsim/I3CLSimClientModule.cxx:513-520), and a count and a
 * weight sum of the photons at DOMs, accumulated over the returned photons behind the particle lookup and the ignoreModules mask
 * (:386-405); the module puts them into the frame at :728-740.  Its weight sums are binary64 running sums -- the generated one of
 * (double)numPhotons * weight, rounded per step -- in arrival order, which no two runs repeat.  THE SUMS BELOW ARE THIS PROJECT'S OWN
 * DEFINITION: exact integers, so that a result is a function of the input as a multiset -- the same bytes whatever the schedule,
 * the wave shape or the bunch partition, from the kernels and from the host twin -- and bunches add exactly.
 * A float weight is w = +-m * 2^(s-149): with e its biased exponent and f its 23 fraction bits, m = f for e = 0 and f | 2^23
 * otherwise (m < 2^24), s = max(e, 1) - 1 (0 ... 253).
 *     at-DOM term      w itself:                    +-m * 2^s                    units of 2^-149
 *     generated term   the EXACT num_photons * w:   +-(num_photons * m) * 2^s    units of 2^-149 (a 56-bit integer, shifted; nothing
 *                      is rounded, where the reference rounds the product to 53 bits)
 * A sum is the integer sum of its terms in units of 2^-149, delivered as six little-endian uint64 words in two's complement.  A
 * bunch holds at most 2^32 - 1 records, so its sum stays below 2^341: 384 bits hold the sum of 2^42 bunches.
 * Terms that are not finite are counted, not summed, in three counters per side: +inf, -inf and NaN terms.  A weight with e = 255
 * is +-inf for f = 0 and NaN otherwise; a generated term with a non-finite weight and num_photons = 0 is a NaN term (0 x inf),
 * one with an infinite weight and num_photons > 0 an inf term of the weight's sign.  The counts (generated_count, at_doms_count)
 * include the records whose terms are not finite, as the reference's do.
 * Per step, all n enqueued steps -- dummy steps and steps the propagator's guards skip included; the reference counts before anything
 * is sent:
 *     its identifier is not in the particle table -> UNKNOWN_STEP_PARTICLE, ignored (the reference skips it silently, :514);
 *     else generated_count += num_photons and the generated term is added.
 * Per photon, in this order:
 *     its identifier is not in the particle table -> UNKNOWN_PARTICLE, not counted (log_fatal in the reference, :388-390);
 *     (frame, string_id, om_id) is in the mask -> MASKED, not counted (:399; not an error);
 *     else at_doms_count += 1 and the at-DOM term is added.
 * No DOM list is needed: a mask entry whose frame no table entry names is ignored, every other one holds for whatever module it names.
 * With a particle table there is one record per table entry, in table order, zeros included (an empty table: no record); without
 * one (particles = NULL) the bunch yields ONE record, identifier 0 and frame 0, every identifier belongs to it, and the mask's frame
 * is 0. */
typedef struct {
    uint32_t identifier, frame;         /* the table entry's */
    uint64_t generated_count;           /* the sum of num_photons */
    uint64_t at_doms_count;
    uint64_t generated_sum[6], at_doms_sum[6];              /* units of 2^-149, least significant word first, two's complement */
    uint32_t generated_special[3], at_doms_special[3];      /* +inf, -inf, NaN terms */
} clsimhip_event_statistics;            /* 144 bytes */
typedef char clsimhip_event_statistics_is_144_bytes[sizeof(clsimhip_event_statistics) == 144 ? 1 : -1];
#define CLSIMHIP_EVENT_STATISTICS_UNKNOWN_PARTICLE 0        /* index into the counters */
#define CLSIMHIP_EVENT_STATISTICS_MASKED 1
#define CLSIMHIP_EVENT_STATISTICS_UNKNOWN_STEP_PARTICLE 2
/* acc += rec: the words of both sums with carry (modulo 2^384), both counts, the six special counters.  acc's identifier and frame
 * stay.  CLSIMHIP_ERR_ARGUMENT for a null pointer. */
int clsimhip_event_statistics_add(clsimhip_event_statistics *acc, const clsimhip_event_statistics *rec);
/* A sum as a binary64: the canonical NaN 0x7ff8000000000000 with NaN terms or inf terms of both signs (or a null pointer), +-inf
 * with inf terms of one sign only, else the integer rounded ONCE to nearest, ties to even, and scaled by 2^-149; zero is +0.0. */
double clsimhip_event_statistics_weight(const uint64_t words[6], const uint32_t special[3]);
/* The host twin.  steps / photons may be NULL with a count of 0; particles = NULL, n_particles = 0: no table; `out` holds
 * n_particles records (one without a table); counters[3] (may be NULL) receives the three counts.  CLSIMHIP_ERR_ARGUMENT for a table
 * that is not strictly increasing in identifier and for more than 2^32 - 1 steps, photons, particles or masked modules. */
int clsimhip_event_statistics_host(const clsimhip_step *steps, size_t n_steps, const clsimhip_photon *photons, size_t n_photons,
                                   const clsimhip_mcpe_particle *particles, size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked,
                                   clsimhip_event_statistics *out, uint64_t counters[3]);
/* bytes of device memory the kernels need beside their input and output, for a bunch with this table and mask */
size_t clsimhip_event_statistics_workspace_bytes(size_t n_particles, size_t n_masked);
/* The kernels, on steps and photon records that live in HBM: n_steps records of d_steps and min(*d_count, capacity) records of
 * d_photons (d_steps may be NULL with n_steps = 0, d_photons with capacity = 0).  d_steps and d_photons 4-byte aligned, d_out
 * (n_particles records, one without a table) 8-byte, d_workspace (clsimhip_event_statistics_workspace_bytes(n_particles, n_masked)
 * bytes) 16-byte, d_count and d_counters 4-byte; d_counters: four uint32 -- the three counters, then the records written
 * (CLSIMHIP_ERR_ARGUMENT for a null or misaligned pointer or a workspace that is too small; nothing is launched then).  The
 * particle table and the mask are host memory: they are checked and copied before the call returns (which may wait for the previous
 * call's copy, nothing else); the kernels are asynchronous on hip_stream (NULL = default stream) and nothing else waits for the
 * device.  One call at a time per process prepares its bunch. */
int clsimhip_event_statistics_device(int device, const void *d_steps, size_t n_steps, const void *d_photons, const void *d_count, size_t capacity,
                                     const clsimhip_mcpe_particle *particles, size_t n_particles, const clsimhip_mcpe_mask *masked, size_t n_masked,
                                     void *d_out, void *d_counters, void *d_workspace, size_t workspace_bytes, void *hip_stream);
/* The stage behind every bunch's propagation kernel, on the bunch's stream: over the bunch's steps as they were uploaded and over
 * ALL detected photons -- with the cable shadow stage bound too: the reference takes its statistics before the shadow module runs.
 * Before Initialize() only (CLSIMHIP_ERR_STATE after).  on = 0 (the default): no launch, no allocation, no byte changes anywhere.
 * With it on, clsimhip_enqueue_steps_with_particles is accepted, it works with keep_photons = 0 under any hit maker, and a bunch
 * with UNKNOWN_PARTICLE > 0 fails as the series stages' do, with the count in the text. */
int clsimhip_set_event_statistics(clsimhip_converter *c, int on);
/* Records of the result `photons` belongs to (one per table entry in table order; one without a table), valid until
 * clsimhip_release_result(c, photons); counters[3] (may be NULL) receives the three counts.  CLSIMHIP_ERR_STATE without
 * clsimhip_set_event_statistics. */
int clsimhip_get_result_event_statistics(clsimhip_converter *c, const clsimhip_photon *photons, const clsimhip_event_statistics **records, size_t *n,
                                         uint64_t counters[3]);

/* ---- Photon hits: stored frame photons -> per-frame, per-DOM time-sorted MCPEs, with the calibration look-ups ------------------
 * The second half of the reference's two-step workflow (python/traysegments/I3CLSimMakeHitsFromPhotons.py): photons are propagated
 * once and stored as PropagatedPhotons -- here clsimhip_frame_photon records with their series table, what the frame photons stage
 * delivers, cable shadow applied if bound -- and hits are made from them as often as needed, with another DOM efficiency or angular
 * acceptance each time.  The module that does it is the older I3PhotonToMCPEConverter (private/clsim/dom/
 * I3PhotonToMCPEConverter.cxx:257-539); this stage restates its per-DOM and per-photon work as a function of the input arrays, a
 * fixed configuration and a 64-bit seed.
 * The efficiency of every DOM is fixed when the maker is made, by the reference's rule (:327-388); its log_fatals there depend on the
 * configuration alone and are CLSIMHIP_ERR_CONFIG here, naming the DOM:
 *     default_relative_efficiency < 0 is an error (:172);
 *     replace_efficiency_with_default: the efficiency is the default; a NaN default is an error;
 *     a DOM not in the calibration (flag bit 1 clear) takes the default; a NaN default is an error;
 *     a DOM in the calibration with a NaN relative_dom_eff takes the default, WITHOUT the SPE factor; a NaN default is an error;
 *     otherwise relative_dom_eff x (isnan(spe_compensation_factor) ? 1 : spe_compensation_factor), one binary64 product.
 * Record i belongs to series s, the last entry of the series table with first <= i (a binary search; nothing checks that `first`
 * ascends).  Per record, in this order:
 *     no such entry, or i >= first + count -> UNCOVERED, no record;
 *     the record's (string_id, om_id) differ from the entry's -> SERIES_MISMATCH, no record;
 *     the DOM is not in the table -> UNKNOWN_DOM (log_fatal in the reference, :295-298);
 *     ignore_inactive and the DOM's flag bit 0 is clear -> INACTIVE, no record (:288-292; not an error);
 *     W = weight; W < 0 -> NEGATIVE_WEIGHT; W == 0 -> nothing (:397-399);
 *     dir = (sin theta cos phi, sin theta sin phi, cos theta) from the deterministic single precision pairs of the MCPE generator,
 *     widened; c = -(dir.x Dx + dir.y Dy + dir.z Dz), then c = c < 1 ? c : 1, c = c > -1 ? c : -1 (:409-412).  D is the DOM's
 *     direction as given, not normalised;
 *     only when pancake == 1: r^2 = x x + y y + z z outside [max(oversize R - 0.03, 0)^2, (oversize R + 0.03)^2], R = dom_radius
 *     -> OFF_SURFACE: counted, and no record unless only_warn_off_surface (:417-453).  Positions are relative to the module, as the
 *     frame photons stage stores them;
 *     P = W x wavelength acceptance of the DOM's class, then x angular acceptance(c), then x efficiency (:466-474);
 *     P > 1 -> PROBABILITY_ABOVE_ONE (:478-504);
 *     u = (h >> 11) 2^-53, h = seed folded with splitmix64 over the record's six little-endian 64-bit words; P <= u -> nothing;
 *     time = record time + ((-x) dir.x + (-y) dir.y + (-z) dir.z) x (1 - pancake / oversize) / group_velocity (:512-518); a NaN is
 *     stored as 0x7ff8000000000000.
 * All of it is binary64 + - x / in the order written, never contracted, so the kernels and the host twin give the same bits for every
 * 48-byte pattern.  Comparisons with a NaN are false: a NaN weight goes on, a NaN c becomes 1, a NaN r^2 is OFF_SURFACE, a NaN P
 * yields a record, a NaN wavelength reads its table's last bin.
 * The kept records come out ascending in (s, tkey(time), identifier) with the MCPE series' tkey; string_id and om_id are the
 * entry's.  The output series table has one entry per input entry that kept a record, in input order, with the entry's frame,
 * string_id and om_id.  Records with equal keys are byte-identical: the output is a function of the input, the same bytes from run
 * to run and from the kernels and the host twin; it has the form clsimhip_mcpe_merge_host / _device read.
 * What differs from the reference, on purpose: the draw (no I3RandomService in arrival order; with one seed the hits made at a lower
 * efficiency are a subset of those made at a higher one); the total order where std::sort(MCPETimeLess) leaves equal times open;
 * CheckSanity (:455) does not apply to compressed photons; merging is the MCPE merging stage's rule, applied by the caller; the
 * cross-checks between I3OMGeo and I3ModuleGeo (:301-325) are the caller's configuration. */
typedef struct {
    int32_t string_id;                  /* must fit int16 / uint16 (CLSIMHIP_ERR_ARGUMENT otherwise); a pair named twice: */
    uint32_t om_id;                     /* CLSIMHIP_ERR_ARGUMENT */
    int32_t class_index;                /* wavelength acceptance class */
    uint32_t flags;                     /* bit 0: has a detector status entry with pmtHV != 0; bit 1: is in the calibration */
    double relative_dom_eff, spe_compensation_factor;       /* the calibration's; NaN where it has none */
    double dir_x, dir_y, dir_z;         /* I3OMGeo::GetDirection() */
} clsimhip_photon_hit_dom;              /* 56 bytes */
typedef struct {
    double dom_radius, oversize, pancake;       /* positive and finite */
    double default_relative_efficiency;         /* may be NaN: "there is no default" */
    int32_t replace_efficiency_with_default, ignore_inactive, only_warn_off_surface, reserved;
    uint64_t seed;
} clsimhip_photon_hit_config;           /* 56 bytes */
typedef char clsimhip_photon_hit_dom_is_56_bytes[sizeof(clsimhip_photon_hit_dom) == 56 ? 1 : -1];
typedef char clsimhip_photon_hit_config_is_56_bytes[sizeof(clsimhip_photon_hit_config) == 56 ? 1 : -1];
#define CLSIMHIP_PHOTON_HITS_FLAG_HAS_STATUS 1u
#define CLSIMHIP_PHOTON_HITS_FLAG_IN_CALIBRATION 2u
#define CLSIMHIP_PHOTON_HITS_UNCOVERED 0            /* index into the seven counters */
#define CLSIMHIP_PHOTON_HITS_SERIES_MISMATCH 1
#define CLSIMHIP_PHOTON_HITS_UNKNOWN_DOM 2
#define CLSIMHIP_PHOTON_HITS_INACTIVE 3
#define CLSIMHIP_PHOTON_HITS_NEGATIVE_WEIGHT 4
#define CLSIMHIP_PHOTON_HITS_OFF_SURFACE 5
#define CLSIMHIP_PHOTON_HITS_PROBABILITY_ABOVE_ONE 6
typedef struct clsimhip_photon_hit_maker clsimhip_photon_hit_maker;
/* n_classes (1 ... 8) wavelength acceptances and the angular acceptance as for clsimhip_mcpe_generator_create, with the same limits;
 * a DOM table of up to 2^24 entries; the configuration.  Host only: no GPU is touched. */
int clsimhip_photon_hit_maker_create(const clsimhip_function *classes, size_t n_classes, const clsimhip_polynomial *angular_acceptance,
                                     const clsimhip_photon_hit_dom *doms, size_t n_doms, const clsimhip_photon_hit_config *config,
                                     clsimhip_photon_hit_maker **out);
void clsimhip_photon_hit_maker_destroy(clsimhip_photon_hit_maker *g);
const char *clsimhip_photon_hit_maker_last_error(const clsimhip_photon_hit_maker *g);
/* the resolved efficiency of a DOM of the table (CLSIMHIP_ERR_ARGUMENT for any other DOM) */
int clsimhip_photon_hit_maker_efficiency(const clsimhip_photon_hit_maker *g, int32_t string_id, uint32_t om_id, double *out);
/* The host twin: the definition with std::sort on the key, for callers without a GPU and for the tests.  out holds n entries,
 * out_series n_series; counters[7] (may be NULL) receives the seven counts. */
int clsimhip_photon_hits_host(const clsimhip_photon_hit_maker *g, const clsimhip_frame_photon *records, size_t n, const clsimhip_mcpe_series *series,
                              size_t n_series, clsimhip_mcpe *out, clsimhip_mcpe_series *out_series, size_t *n_kept, size_t *n_series_out,
                              uint64_t counters[7]);
/* bytes of device memory the kernels need beside their input and output, for up to `capacity` records */
size_t clsimhip_photon_hits_workspace_bytes(size_t capacity);
/* The kernels, on frame photons that live in HBM (pairs with clsimhip_frame_photons_device: d_records = its d_out, d_series = its
 * d_series, d_in_counts = its d_counts, whose first two words are records kept and series): min(d_in_counts[0], capacity) records,
 * min(d_in_counts[1], capacity) series entries.  d_out and d_out_series: `capacity` entries each; d_records, d_series, d_out,
 * d_out_series and d_workspace (clsimhip_photon_hits_workspace_bytes(capacity) bytes) 16-byte aligned, d_in_counts and d_counts
 * 4-byte; d_counts: nine uint32 -- records kept, series, then the seven counters (CLSIMHIP_ERR_ARGUMENT for a null or misaligned
 * pointer or a workspace that is too small; nothing is launched then).  The kernels are asynchronous on hip_stream (NULL = default
 * stream) and read all sizes from device memory; the first call on a device copies the maker's tables there, nothing else waits for
 * the device. */
int clsimhip_photon_hits_device(clsimhip_photon_hit_maker *g, int device, const void *d_records, const void *d_series, const void *d_in_counts,
                                size_t capacity, void *d_out, void *d_out_series, void *d_counts, void *d_workspace, size_t workspace_bytes,
                                void *hip_stream);

/* ---- PMT photon hits: stored frame photons -> per-frame, per-module, per-PMT time-sorted hits of segmented modules ---------------
 * The reference's hit maker for segmented modules, I3PhotonToMCHitConverterForMultiPMT::DAQ (private/clsim/dom/
 * I3PhotonToMCHitConverterForMultiPMT.cxx:244-407), is an offline module: it reads a stored I3PhotonSeriesMap, finds for every
 * (module, photon) the hit PMT, draws, files the hit under OMKey and PMT number and time-sorts every PMT's vector.  This stage is that
 * module on clsimhip_frame_photon records with their series table (what the frame photons stage delivers, cable shadow applied if
 * bound), with the tables, the module list and the seed of a clsimhip_pmt_generator: photons are propagated once, hits are made as
 * often as needed with another quantum efficiency, collection efficiency or angular acceptance.  Stand-alone, like the photon hits
 * stage; no converter runs it.
 * Record i belongs to series s, the last entry of the series table with first <= i (a binary search; nothing checks that `first`
 * ascends).  Per record, in this order:
 *     no such entry, or i >= first + count -> UNCOVERED, no hit;
 *     the record's (string_id, om_id) differ from the entry's -> SERIES_MISMATCH, no hit;
 *     the module is not one of the generator's -> UNKNOWN_MODULE (log_fatal in the reference, :281-283);
 *     the generator's geometry and probability, on the record's x, y, z (relative to the module), theta, phi, wavelength and weight:
 *     a photon that is leaving makes no hit; r^2 outside the type's 3 cm window -> OFF_SURFACE, counted, and the record goes on; the
 *     PMT met from the front at the shortest path, none -> no hit; P = W x G(wavelength) x Q(wavelength) ce x A(c) / c;
 *     P > 1 -> PROBABILITY_ABOVE_ONE (log_fatal in the reference, :348-351);
 *     u = (h >> 11) 2^-53, h = the generator's seed folded with splitmix64 over the record's six little-endian 64-bit words;
 *     P <= u -> no hit;
 *     hit = {identifier, string_id, om_id, pmt, reserved 0, time}: the time is the record's, bit for bit (it carries the
 *     particle's shift already; no arithmetic, so a NaN keeps its sign and payload).
 * All of it is binary64 + - x / in the order written, never contracted, so the kernels and the host twin give the same bits for every
 * 48-byte pattern.  Comparisons with a NaN are false, as for the generator: a NaN direction ends on the type's last PMT, a NaN weight
 * or P yields a hit.
 * The kept hits come out ascending in (s, pmt, tkey(time), identifier) with the MCPE series' tkey (the key's group is s x 64 + pmt,
 * so s must stay below 2^26).  The output series table has one clsimhip_pmt_series entry {frame, string_id, om_id, pmt, first, count,
 * 0} per non-empty (s, pmt) in the same order, with the input entry's frame and IDs; its entries partition the hits.  Hits with equal
 * keys are byte-identical: the output is a function of the input, the same bytes from run to run and from the kernels and the host
 * twin.
 * What differs from the reference, on purpose: the draw (no I3RandomService in arrival order; with one seed the hits made at a lower
 * collection efficiency are a subset of those made at a higher one); the total order where std::sort(MCHitTimeLess) leaves equal
 * times open; the path-length argument of the glass / gel survival is not modelled, as for the generator; the MCTree lookup
 * (:356-360) is the caller's: the hit carries the identifier.  Not pinned against the reference's output, like the rest of the
 * multi-PMT hit maker (I3OMTypeInfo and I3Orientation are outside it). */
#define CLSIMHIP_PMT_PHOTON_HITS_UNCOVERED 0            /* index into the five counters */
#define CLSIMHIP_PMT_PHOTON_HITS_SERIES_MISMATCH 1
#define CLSIMHIP_PMT_PHOTON_HITS_UNKNOWN_MODULE 2
#define CLSIMHIP_PMT_PHOTON_HITS_PROBABILITY_ABOVE_ONE 3
#define CLSIMHIP_PMT_PHOTON_HITS_OFF_SURFACE 4
/* The host twin: the definition with std::sort on the key, for callers without a GPU and for the tests.  out and out_series hold n
 * entries each; counters[5] (may be NULL) receives the five counts.  CLSIMHIP_ERR_ARGUMENT for n_series > 2^26. */
int clsimhip_pmt_photon_hits_host(const clsimhip_pmt_generator *g, const clsimhip_frame_photon *records, size_t n, const clsimhip_mcpe_series *series,
                                  size_t n_series, clsimhip_pmt_hit *out, clsimhip_pmt_series *out_series, size_t *n_kept, size_t *n_series_out,
                                  uint64_t counters[5]);
/* bytes of device memory the kernels need beside their input and output, for up to `capacity` records */
size_t clsimhip_pmt_photon_hits_workspace_bytes(size_t capacity);
/* The kernels, on frame photons that live in HBM (pairs with clsimhip_frame_photons_device: d_records = its d_out, d_series = its
 * d_series, d_in_counts = its d_counts, whose first two words are records kept and series): min(d_in_counts[0], capacity) records,
 * min(d_in_counts[1], capacity) series entries.  d_out and d_out_series: `capacity` entries each; d_records, d_series, d_out,
 * d_out_series and d_workspace (clsimhip_pmt_photon_hits_workspace_bytes(capacity) bytes) 16-byte aligned, d_in_counts and d_counts
 * 4-byte; d_counts: seven uint32 -- hits kept, series, then the five counters (CLSIMHIP_ERR_ARGUMENT for a null or misaligned
 * pointer, a workspace that is too small or capacity > 2^26; nothing is launched then).  The kernels are asynchronous on hip_stream
 * (NULL = default stream) and read all sizes from device memory; the generator's tables on the device are those
 * clsimhip_pmt_convert_device uses (the first of the two calls on a device copies them there), nothing else waits for the device. */
int clsimhip_pmt_photon_hits_device(clsimhip_pmt_generator *g, int device, const void *d_records, const void *d_series, const void *d_in_counts,
                                    size_t capacity, void *d_out, void *d_out_series, void *d_counts, void *d_workspace, size_t workspace_bytes,
                                    void *hip_stream);

/* ---- Muon slicer: a muon with a length becomes slices between its stochastic losses ------------------------------------------
 * The reference's standard chain cuts every muon that has a length into slices between its daughters (I3MuonSlicer,
 * private/clsim/util/I3MuonSlicer.cxx:182-493 and the primaries loop :531-555); each slice carries the energy the muon still has
 * there, and slices and cascades are propagated as light sources of their own.  Here: sequential binary64 host code on a flattened
 * tree, every formula in the reference's operation order (dEdt_calc, dEdt_max with its one log, their min, the running energy and
 * time, the reset to 0 at :319-322), in this library's units (m, ns, GeV; c = 0.299792458 m/ns).
 * INPUT: the tree in depth-first pre-order -- a node's children follow it, in the reference's sibling order; parent < own index.
 * OUTPUT: the reference's append order, pre-order as well.  A sliced muon comes first, with CLSIMHIP_TREE_DARK set; then, per
 *     daughter, the slice in front of it (if its length >= 0.1 mm), the daughter, and the daughter's own sliced subtree; the slice
 *     behind the last daughter comes last.  A slice copies the muon's type, shape, flags as they were on input, direction and speed,
 *     and takes identifier = first_slice_identifier + k, k its position among the slices in output order; `relabel` receives
 *     (that identifier -> the muon's identifier), strictly ascending in `from` by construction.
 * The paths without slices are the reference's: a muon that is not in `tracks`, or whose Ei / Ef are invalid, takes the particle's
 *     own values (:257-268); the early returns at :421-434 and :441-444; tf < ti and tf == ti only darken the muon; a muon without a
 *     length, and any other particle, is copied and recursed into.  A daughter more than 1 mm off the track is appended and skipped
 *     (its subtree with it, :326-333); a daughter with a NaN time is dropped (:335).
 * The reference's log_fatal conditions are CLSIMHIP_ERR_ARGUMENT, with text that names the first offending node, and nothing is
 *     written: a muon or a type-0 daughter below a muon with a length; NaN speed, energy or time of such a muon; daughters not
 *     ascending in time (the reference's own check never clears its first-iteration flag and so only ever refuses NaN times; here it
 *     is what its text says: a NaN time of the first daughter, or a time below the predecessor's); Ei <= 0 with daughters; an
 *     identifier twice in `tracks`.  Also refused: parent >= index, a slice identifier that equals an input identifier, slice
 *     identifiers that would wrap.
 * counters[5] (may be NULL): what the reference logs as error or warning -- OFF_TRACK, ENERGY_RESET, STOPS_BEFORE_START,
 *     ZERO_DURATION, LONG_SLICE (> 1 km).
 * *n_out and *n_relabel are what is needed; at most the capacities are written, as clsimhip_ppc_enqueue does it.  A caller passes
 * clsimhip_ppc_enqueue the output nodes without CLSIMHIP_TREE_DARK.  The block under TRY_TO_CORRECT_MMC is compiled out upstream
 * and is not here.  Host only, no GPU is touched. */
#define CLSIMHIP_TREE_DARK 1u                 /* I3Particle::Dark */
#define CLSIMHIP_SLICER_OFF_TRACK 0           /* index into the five counters */
#define CLSIMHIP_SLICER_ENERGY_RESET 1
#define CLSIMHIP_SLICER_STOPS_BEFORE_START 2
#define CLSIMHIP_SLICER_ZERO_DURATION 3
#define CLSIMHIP_SLICER_LONG_SLICE 4
typedef struct {
    clsimhip_particle particle;               /* as clsimhip_ppc_enqueue takes it */
    double speed;                             /* [m/ns] */
    int32_t parent;                           /* index of the parent in the same array, -1: a primary; parent < own index */
    uint32_t flags;                           /* CLSIMHIP_TREE_* */
} clsimhip_tree_particle;                     /* 104 bytes */
typedef struct { uint32_t identifier, reserved; double Ei, Ef, ti, tf; } clsimhip_mmc_track;   /* 40 bytes */
typedef struct { uint32_t from, to; } clsimhip_relabel;                                        /* 8 bytes */
typedef char clsimhip_tree_particle_is_104_bytes[sizeof(clsimhip_tree_particle) == 104 ? 1 : -1];
typedef char clsimhip_mmc_track_is_40_bytes[sizeof(clsimhip_mmc_track) == 40 ? 1 : -1];
typedef char clsimhip_relabel_is_8_bytes[sizeof(clsimhip_relabel) == 8 ? 1 : -1];
int clsimhip_slice_muons(const clsimhip_tree_particle *tree, size_t n, const clsimhip_mmc_track *tracks, size_t n_tracks,
                         uint32_t first_slice_identifier, clsimhip_tree_particle *out, size_t capacity, size_t *n_out,
                         clsimhip_relabel *relabel, size_t relabel_capacity, size_t *n_relabel, uint64_t counters[5]);

/* ---- Series relabel: records take their muon's identifier, and the series form's order is restored -------------------------
 * Behind its hit makers the reference replaces every slice's identifier, in every MCPE and every photon, by that of the muon the
 * slice was cut from (I3MuonSliceRemoverAndPulseRelabeler, private/clsim/util/I3MuonSliceRemoverAndPulseRelabeler.cxx:230-400).
 * The series forms here end their key in the identifier, so the order has to be made again:
 * RELABEL(X, map) for a series form X of MCPEs or of frame photons: every record whose identifier is a `from` of the map takes that
 *     entry's `to`; all other bytes stay; the series table is unchanged; the records of every series are put back into the form's
 *     order.  Only runs of records equal in (series entry, tkey) can be out of order.  A run is DISTURBED when its new identifiers
 *     descend somewhere.  Undisturbed runs are copied, whatever their length.  A disturbed run is sorted on the rest of the key:
 *     `identifier` for MCPEs; `identifier, h, w0 ... w7` for frame photons, h as the frame photon contract defines it.  A disturbed
 *     run of more than 2 048 records is counted member by member as TIE_OVERFLOW, and the call then delivers nothing (records =
 *     series = 0): loud, as for the frame photon stage.
 * The map is strictly ascending in `from`, and no `to` may equal any `from` (the reference's own sanity check, :320-332); a map that
 * breaks either rule is CLSIMHIP_ERR_ARGUMENT.  An empty map gives a copy.  Equal keys are equal bytes for both record types, so the
 * result is a function of the input: the same bytes from the host twins and the kernels.
 * The host twins (a walk over the runs, std::stable_sort; host only, no GPU is touched): a malformed input is CLSIMHIP_ERR_ARGUMENT.
 * out_records holds n entries; counters[2] (may be NULL): RELABELLED, TIE_OVERFLOW; *n_kept: n, or 0 after a TIE_OVERFLOW. */
#define CLSIMHIP_RELABEL_RELABELLED 0         /* index into the two counters */
#define CLSIMHIP_RELABEL_TIE_OVERFLOW 1
int clsimhip_mcpe_series_relabel_host(const clsimhip_mcpe *records, size_t n, const clsimhip_mcpe_series *series, size_t n_series,
                                      const clsimhip_relabel *map, size_t n_map, clsimhip_mcpe *out_records, uint64_t counters[2], size_t *n_kept);
int clsimhip_frame_photons_relabel_host(const clsimhip_frame_photon *records, size_t n, const clsimhip_mcpe_series *series, size_t n_series,
                                        const clsimhip_relabel *map, size_t n_map, clsimhip_frame_photon *out_records, uint64_t counters[2],
                                        size_t *n_kept);
/* bytes of device memory the kernels need beside their input and output (the map's copy included); record_bytes: 16 (MCPEs) or 48
 * (frame photons), anything else: 0 */
size_t clsimhip_series_relabel_workspace_bytes(size_t capacity, size_t n_map, size_t record_bytes);
/* The kernels, on series that live in HBM.  The input is read as clsimhip_mcpe_merge_device reads it: min(counts[0], capacity)
 * records, min(counts[1], capacity) series; it is taken as a series form and not checked again.  d_out_records and d_out_series:
 * `capacity` entries each; d_out_series receives a copy of the table, so the output triple is complete; d_out_counts: five uint32 --
 * records, series, RELABELLED, 0, TIE_OVERFLOW; the first two follow the series stage's layout, so the output chains unchanged into
 * the merge, a union, a split and a store's add_device.  The map is host memory; it is checked and copied before the call returns, as
 * the series stage treats its particle table.  Whatever bytes the input holds, nothing is written beyond a capacity and every loop
 * is bounded by one.  The output must not overlap the input (CLSIMHIP_ERR_ARGUMENT).  Records, tables and d_workspace
 * (clsimhip_series_relabel_workspace_bytes bytes) are 16-byte aligned, the counts 4-byte; capacity is at most 2^31.  Asynchronous on
 * hip_stream (NULL = default stream); nothing waits for the device. */
int clsimhip_mcpe_series_relabel_device(int device, const void *d_records, const void *d_series, const void *d_counts, size_t capacity,
                                        const clsimhip_relabel *map, size_t n_map, void *d_out_records, void *d_out_series,
                                        void *d_out_counts, void *d_workspace, size_t workspace_bytes, void *hip_stream);
int clsimhip_frame_photons_relabel_device(int device, const void *d_records, const void *d_series, const void *d_counts, size_t capacity,
                                          const clsimhip_relabel *map, size_t n_map, void *d_out_records, void *d_out_series,
                                          void *d_out_counts, void *d_workspace, size_t workspace_bytes, void *hip_stream);
/* The merging stage's parent table under the map, host only: per range the identifiers are replaced, the entries sorted by
 * (identifier, index), duplicates dropped and the ranges rebuilt (the ranges must lie end to end; out holds as many entries as the
 * input, out_ranges n_series).  The reference's version of this step tests the wrong way round (:369-370) and dereferences end() for
 * every particle that is not a slice; that defect is not restated.  On the device there is no such stage: merging ignores particles,
 * so the parent table comes from running clsimhip_mcpe_merge_device BEHIND the relabel stage. */
int clsimhip_mcpe_parents_relabel_host(const clsimhip_mcpe_parent *parents, const clsimhip_mcpe_parent_range *ranges, size_t n_series,
                                       const clsimhip_relabel *map, size_t n_map, clsimhip_mcpe_parent *out,
                                       clsimhip_mcpe_parent_range *out_ranges, size_t *n_out);

/* ---- Event statistics frame store: per frame and per particle, the exact sums of bunch after bunch ----------------------------
 * The client module of the reference files four things into a frame: MCPEs, frame photons, PMT hits and I3CLSimEventStatistics
 * (private/clsim/I3CLSimClientModule.cxx:728-740).  The first three have their frame stores above; this is the fourth.  A frame's light
 * spans several bunches, and with muon slicing the particle table holds one entry per slice, while the user wants one record per
 * muon and frame.  The sums are exact integers modulo 2^384 and the counts are modular too, so addition is associative and
 * commutative, and the content of a store is a function of the multiset of records it was given: the same bytes whatever order the
 * bunches arrive in, from the host twins and from the kernels.
 * KEY of a record: (frame, identifier), compared as two unsigned 32-bit integers, frame first.
 * EMPTY record: the 136 bytes behind identifier and frame are all zero.
 * STATISTICS FORM: n records of clsimhip_event_statistics, strictly ascending in the key, none empty.  A record that is empty, or whose
 *     key is not above its predecessor's, is one MALFORMED element.
 * ADD: clsimhip_event_statistics_add -- sum words with carry modulo 2^384, counts modulo 2^64, special counters modulo 2^32.
 * CANON(L, map) for any list L of records, in any key order, duplicates and empties allowed: drop the empty records (EMPTY_DROPPED);
 *     replace every identifier that is a `from` of the map by its `to` (RELABELLED; the frame stays); sort by key; replace every run
 *     of equal keys by its ADD-sum, carrying the key.  The result is a statistics form.  The map follows the series relabel stage's
 *     rules (strictly ascending in `from`, no `to` equal to any `from`, CLSIMHIP_ERR_ARGUMENT otherwise; an empty map is allowed).  A run
 *     may be as long as the input: addition needs no order inside a run, so there is no tie limit.
 * COMBINE(A, B) of two statistics forms: merged by key, equal keys become one record by ADD; n_out <= n_a + n_b.
 * SPLIT(X, last_frame): the head is the prefix with frame <= last_frame, the tail the rest; 0xFFFFFFFF drains everything.
 * From these: COMBINE(A, B) = COMBINE(B, A); COMBINE(CANON(L1), CANON(L2)) = CANON(L1 ++ L2); CANON(CANON(L, no map), map) =
 * CANON(L, map) -- folding the slices when a bunch is added and folding them when a frame is drained give the same bytes.
 * The host twins (host only, no GPU is touched): malformed input or an output that does not fit is CLSIMHIP_ERR_ARGUMENT, with text
 * that names the first offending element, and nothing is written.  counters[2] (may be NULL): RELABELLED, EMPTY_DROPPED. */
#define CLSIMHIP_EVENT_STATISTICS_STORE_RELABELLED 0      /* index into the two counters */
#define CLSIMHIP_EVENT_STATISTICS_STORE_EMPTY_DROPPED 1
int clsimhip_event_statistics_canonical_host(const clsimhip_event_statistics *records, size_t n, const clsimhip_relabel *map, size_t n_map,
                                             clsimhip_event_statistics *out, size_t capacity, size_t *n_out, uint64_t counters[2]);
int clsimhip_event_statistics_combine_host(const clsimhip_event_statistics *a, size_t n_a, const clsimhip_event_statistics *b, size_t n_b,
                                           clsimhip_event_statistics *out, size_t capacity, size_t *n_out);
int clsimhip_event_statistics_split_host(const clsimhip_event_statistics *records, size_t n, uint32_t last_frame,
                                         clsimhip_event_statistics *head, size_t head_capacity, size_t *n_head,
                                         clsimhip_event_statistics *tail, size_t tail_capacity, size_t *n_tail);
/* bytes of device memory the kernels need beside their inputs and outputs: COMBINE of (capacity_a, capacity_b); CANON of `capacity`
 * records under a map of n_map entries takes (capacity, n_map), the map's copy included */
size_t clsimhip_event_statistics_store_workspace_bytes(size_t capacity_a, size_t capacity_b);
/* The kernels, on records that live in HBM, under the contract of clsimhip_mcpe_series_union_device: an input is read as
 * min(*d_count, capacity) records, its count ONE uint32 in device memory -- word 3 of clsimhip_event_statistics_device's d_counters
 * (the records written) chains in unchanged, and so does word 0 of another stage's output counts; records and d_workspace are
 * 16-byte aligned, counts 4-byte; capacities are at most 2^31; the output must not overlap an input (CLSIMHIP_ERR_ARGUMENT);
 * asynchronous on hip_stream (NULL = default stream), nothing waits for the device; whatever bytes the inputs hold, nothing is
 * written beyond a capacity and every loop is bounded by one.  The map is host memory: it is checked and copied before the call
 * returns.  Output counts are five uint32 in the union's layout:
 *     CANON     records, 0, RELABELLED, EMPTY_DROPPED, overflow -- a result that does not fit delivers nothing (records = 0) and
 *               reports the size it needs;
 *     COMBINE   records, 0, MALFORMED elements in A, MALFORMED elements in B, overflow (the needed size when the result does not fit,
 *               else 0).  B malformed, or a result that does not fit: the output is A unchanged.  A malformed: the output is empty.
 *     SPLIT     head: records, 0, 0, 0, overflow -- a head that does not fit drains nothing and reports the size it needs; tail:
 *               records, 0, 0, 0, 0.  tail_capacity must not be below capacity.  The input is taken as a statistics form. */
int clsimhip_event_statistics_canonical_device(int device, const void *d_records, const void *d_count, size_t capacity,
                                               const clsimhip_relabel *map, size_t n_map, void *d_out, void *d_out_counts, size_t out_capacity,
                                               void *d_workspace, size_t workspace_bytes, void *hip_stream);
int clsimhip_event_statistics_combine_device(int device, const void *d_a, const void *d_a_count, size_t capacity_a, const void *d_b,
                                             const void *d_b_count, size_t capacity_b, void *d_out, void *d_out_counts, size_t out_capacity,
                                             void *d_workspace, size_t workspace_bytes, void *hip_stream);
int clsimhip_event_statistics_split_device(int device, const void *d_records, const void *d_count, size_t capacity, uint32_t last_frame,
                                           void *d_head, void *d_head_counts, size_t head_capacity, void *d_tail, void *d_tail_counts,
                                           size_t tail_capacity, void *hip_stream);
/* THE STORE: add is COMBINE(store, CANON(bunch, map)) -- the bunch is any list of records, a result's records as they come, zeros
 * included; drain delivers CANON(head of SPLIT(store, last_frame), map), and the tail becomes the store.  device < 0: a host store,
 * which needs no GPU and takes no device call (CLSIMHIP_ERR_STATE).  Everything else is as the MCPE frame store documents it: two
 * buffers used in turn; one event orders operations issued on different streams; five sticky counters (malformed bunches, their
 * elements, bunches that did not fit, their records, malformed elements of the store itself), with _size and both drains returning
 * CLSIMHIP_ERR_DEVICE while any is nonzero; add_host validates before anything moves and leaves the store unchanged on refusal (a host
 * store also when the result would exceed its capacity); add_device drops a bunch whose result does not fit, whole, and counts it.
 * _size and the capacity a drain asks of its output are those of the head BEFORE the drain's map folds it; the drain's d_counts are
 * CANON's (records, 0, RELABELLED, EMPTY_DROPPED, overflow), with the split's overflow passed on. */
typedef struct clsimhip_event_statistics_store clsimhip_event_statistics_store;
int clsimhip_event_statistics_store_create(int device, size_t capacity, clsimhip_event_statistics_store **out);
void clsimhip_event_statistics_store_destroy(clsimhip_event_statistics_store *s);
const char *clsimhip_event_statistics_store_last_error(const clsimhip_event_statistics_store *s);
int clsimhip_event_statistics_store_add_host(clsimhip_event_statistics_store *s, const clsimhip_event_statistics *records, size_t n,
                                             const clsimhip_relabel *map, size_t n_map);
int clsimhip_event_statistics_store_add_device(clsimhip_event_statistics_store *s, const void *d_records, const void *d_count, size_t capacity,
                                               const clsimhip_relabel *map, size_t n_map, void *hip_stream);
int clsimhip_event_statistics_store_drain_device(clsimhip_event_statistics_store *s, uint32_t last_frame, const clsimhip_relabel *map,
                                                 size_t n_map, void *d_out, void *d_counts, size_t capacity, void *hip_stream);
int clsimhip_event_statistics_store_drain_host(clsimhip_event_statistics_store *s, uint32_t last_frame, const clsimhip_relabel *map,
                                               size_t n_map, clsimhip_event_statistics *out, size_t capacity, size_t *n);
int clsimhip_event_statistics_store_size(clsimhip_event_statistics_store *s, uint32_t last_frame, size_t *n);

#ifdef __cplusplus
}
#endif
#endif
