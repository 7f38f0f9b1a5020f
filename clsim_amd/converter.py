"""Host-side mirror of the reference's converter interface over the C ABI.

Names, argument meaning and error behaviour follow
  public/clsim/I3CLSimStepToPhotonConverter.h:67-192 and
  public/clsim/I3CLSimStepToPhotonConverterOpenCL.h:78-258;
the helpers follow python/MakeIceCubeMediumProperties.py,
python/GetIceCubeDOMAcceptance.py and I3CLSimModuleHelper.cxx:175-372.
Everything numerical happens inside libclsimhip.so (C++/HIP); this module only
marshals numpy arrays.
"""
import ctypes as C
import math
import os

import numpy as np

from . import _lib
from .synthetic import PHOTON_DTYPE, STEP_DTYPE

NANOMETER = 1e-9


class I3CLSimStepToPhotonConverter_exception(RuntimeError):
    """public/clsim/I3CLSimStepToPhotonConverter.h:57-65"""

    def __init__(self, msg, code=0):
        RuntimeError.__init__(self, msg)
        self.code = code


def _check(rc, handle=None):
    if rc != _lib.OK:
        msg = _lib.load().clsimhip_last_error(handle)
        raise I3CLSimStepToPhotonConverter_exception((msg or b"").decode() or ("status %d" % rc), rc)


def _dp(a):
    return a.ctypes.data_as(_lib.DP)


class I3CLSimFunctionFromTable:
    """private/clsim/function/I3CLSimFunctionFromTable.cxx: (startWlen, wlenStep, values) :70-90, equal spacing, or
    (wlens, values) :57-70, the table's own wavelengths -- host side only, like the reference (:169-170): an emission
    spectrum for makeWavelengthGenerator."""

    def __init__(self, *args):
        if len(args) == 3:
            self.startWlen, self.wlenStep = float(args[0]), float(args[1])
            self.values = np.ascontiguousarray(args[2], dtype=np.float64)
            self.wlens = None
        elif len(args) == 2:
            self.wlens = np.ascontiguousarray(args[0], dtype=np.float64)
            self.values = np.ascontiguousarray(args[1], dtype=np.float64)
            if len(self.wlens) < 2:
                raise I3CLSimStepToPhotonConverter_exception("wlens must contain at least 2 elements!")
            if len(self.wlens) != len(self.values):
                raise I3CLSimStepToPhotonConverter_exception("wlens and values must have the same size!")
        else:
            raise TypeError("I3CLSimFunctionFromTable(startWlen, wlenStep, values) or (wlens, values)")

    def GetInEqualSpacingMode(self):
        return self.wlens is None

    def _desc(self):
        if self.wlens is None:
            return _lib.Function(0, len(self.values), self.startWlen, self.wlenStep, _dp(self.values), 0.0, None)
        return _lib.Function(2, len(self.values), 0.0, 0.0, _dp(self.values), 0.0, _dp(self.wlens))


class I3CLSimFunctionDeltaPeak:
    """function/I3CLSimFunctionDeltaPeak: a single-wavelength emission spectrum (the standard candles)"""

    def __init__(self, peakPosition):
        self.peakPosition = float(peakPosition)

    def GetPeakPosition(self):
        return self.peakPosition

    def _desc(self):
        return _lib.Function(3, 0, 0.0, 0.0, None, self.peakPosition, None)


class I3CLSimFunctionConstant:
    def __init__(self, value):
        self.value = float(value)

    def _desc(self):
        return _lib.Function(1, 0, 0.0, 0.0, None, self.value, None)


class I3CLSimRandomValueInterpolatedDistribution:
    """...InterpolatedDistribution.cxx: (xFirst, xSpacing, y) :57-74, or (x, y) :40-55."""

    def __init__(self, *args):
        if len(args) == 3:
            self.first, self.spacing = float(args[0]), float(args[1])
            self.y = np.ascontiguousarray(args[2], dtype=np.float64)
            self.x = None
        elif len(args) == 2:
            self.x = np.ascontiguousarray(args[0], dtype=np.float64)
            self.y = np.ascontiguousarray(args[1], dtype=np.float64)
            if len(self.x) != len(self.y):
                raise I3CLSimStepToPhotonConverter_exception('The "x" and "y" vectors must have the same size!')
        else:
            raise TypeError("I3CLSimRandomValueInterpolatedDistribution(xFirst, xSpacing, y) or (x, y)")

    def _desc(self):
        if self.x is None:
            return _lib.RandomValue(0, len(self.y), self.first, self.spacing, _dp(self.y), 0.0, None)
        return _lib.RandomValue(3, len(self.y), 0.0, 0.0, _dp(self.y), 0.0, _dp(self.x))


class I3CLSimRandomValueWlenCherenkovNoDispersion:
    """random_value/I3CLSimRandomValueWlenCherenkovNoDispersion.cxx:40-98: 1/lambda uniform between 1/toWlen and 1/fromWlen."""

    def __init__(self, fromWlen, toWlen):
        self.fromWlen, self.toWlen = float(fromWlen), float(toWlen)

    def _desc(self):
        return _lib.RandomValue(2, 0, self.fromWlen, self.toWlen, None, 0.0, None)


class I3CLSimRandomValueConstant:
    def __init__(self, value):
        self.value = float(value)

    def _desc(self):
        return _lib.RandomValue(1, 0, 0.0, 0.0, None, self.value, None)


class I3CLSimMediumProperties:
    """Opaque medium object living in the library (clsimhip_medium)."""

    def __init__(self, handle, keep=None):
        self._h = handle
        self._keep = keep

    def __del__(self):
        try:
            if self._h:
                _lib.load().clsimhip_medium_destroy(self._h)
        except Exception:
            pass

    def describe(self):
        d = _lib.MediumDesc()
        _check(_lib.load().clsimhip_medium_describe(self._h, C.byref(d)))
        nl = d.num_layers

        def arr(p, n):
            return np.ctypeslib.as_array(p, shape=(n,)).copy() if (p and n) else np.zeros(0)
        out = {k: getattr(d, k) for k in ("num_layers", "layers_z_start", "layers_height", "min_wavelength",
                                          "max_wavelength", "lengths_kind", "alpha", "kappa", "A", "B", "D", "E",
                                          "scatter_kind", "liu_fraction", "mean_cosine", "has_anisotropy",
                                          "aniso_azimuth", "aniso_k1", "aniso_k2", "has_pre_transform",
                                          "pre_renormalize", "has_post_transform", "post_renormalize", "has_tilt",
                                          "tilt_azimuth")}
        out["n"] = list(d.n); out["g"] = list(d.g)
        out["pre_matrix"] = np.array(list(d.pre_matrix)).reshape(3, 3)
        out["post_matrix"] = np.array(list(d.post_matrix)).reshape(3, 3)
        out["phase_index_kind"], out["group_index_kind"] = d.phase_index_kind, d.group_index_kind
        for key in ("phase_index_table", "group_index_table"):
            f = getattr(d, key)
            if getattr(d, key.replace("_table", "_kind")) == 1:
                out[key] = dict(start=f.start, step=f.step, values=arr(f.values, f.n))
        if d.lengths_kind == 0:
            out["abs_length"] = arr(d.abs_length, nl); out["sca_length"] = arr(d.sca_length, nl)
        elif d.lengths_kind == 2:
            nw = d.table_num_wavelengths
            out.update(table_num_wavelengths=nw, table_start_wavelength=d.table_start_wavelength,
                       table_wavelength_step=d.table_wavelength_step, table_store_as_16bit=bool(d.table_store_as_16bit))
            out["abs_length_table"] = arr(d.abs_length_table, nl * nw).reshape(nl, nw)
            out["sca_length_table"] = arr(d.sca_length_table, nl * nw).reshape(nl, nw)
        else:
            out["a_dust400"] = arr(d.a_dust400, nl); out["delta_tau"] = arr(d.delta_tau, nl); out["b400"] = arr(d.b400, nl)
        if d.has_tilt:
            nd, nz = d.tilt_num_distances, d.tilt_num_z
            out["tilt_distances"] = arr(d.tilt_distances, nd)
            out["tilt_z_coordinates"] = arr(d.tilt_z_coordinates, nz)
            out["tilt_z_corrections"] = arr(d.tilt_z_corrections, nd * nz).reshape(nd, nz)
        return out


def MakeIceCubeMediumProperties(detectorCenterDepth=1948.07, iceDataDirectory=None, useTiltIfAvailable=True):
    """python/MakeIceCubeMediumProperties.py:49-256 (PPC ice tables -> medium)."""
    h = C.c_void_p()
    _check(_lib.load().clsimhip_medium_create_from_ppc(str(iceDataDirectory).encode(), float(detectorCenterDepth),
                                                        1 if useTiltIfAvailable else 0, C.byref(h)))
    return I3CLSimMediumProperties(h)


def MakeIceCubeMediumPropertiesPhotonics(tableFile, detectorCenterDepth=1948.07):
    """python/MakeIceCubeMediumPropertiesPhotonics.py:47-227 (photonics ice table -> medium)."""
    h = C.c_void_p()
    _check(_lib.load().clsimhip_medium_create_from_photonics(str(tableFile).encode(), float(detectorCenterDepth), C.byref(h)))
    return I3CLSimMediumProperties(h)


def MakeHomogeneousMediumProperties(absLen=100.0, scaLen=25.0, zStart=-1000.0, height=2000.0, meanCosine=0.9,
                                    liuFraction=0.45):
    """BASELINE config C1: one layer with I3CLSimFunctionConstant absorption /
    scattering lengths, IceCube refractive index (SURVEY.md 9.7 option i)."""
    d = _lib.MediumDesc()
    d.num_layers = 1
    d.layers_z_start, d.layers_height = zStart, height
    d.min_wavelength, d.max_wavelength = 265.0 * NANOMETER, 675.0 * NANOMETER
    d.lengths_kind = 0
    a = np.array([absLen], dtype=np.float64); s = np.array([scaLen], dtype=np.float64)
    d.abs_length, d.sca_length = _dp(a), _dp(s)
    for i, v in enumerate((1.55749, -1.57988, 3.99993, -4.68271, 2.09354)):
        d.n[i] = v
    for i, v in enumerate((1.227106, -0.954648, 1.42568, -0.711832, 0.0)):
        d.g[i] = v
    d.scatter_kind = 2
    d.liu_fraction, d.mean_cosine = liuFraction, meanCosine
    h = C.c_void_p()
    _check(_lib.load().clsimhip_medium_create(C.byref(d), C.byref(h)))
    return I3CLSimMediumProperties(h)


def GetIceCubeDOMAcceptance(domRadius=0.16510, efficiency=1.0):
    """python/GetIceCubeDOMAcceptance.py:35-115."""
    vals = np.zeros(43, dtype=np.float64)
    start, step = C.c_double(), C.c_double()
    _check(_lib.load().clsimhip_icecube_dom_acceptance(domRadius, efficiency, _dp(vals), C.byref(start), C.byref(step)))
    return I3CLSimFunctionFromTable(start.value, step.value, vals)


def makeCherenkovWavelengthGenerator(wavelengthGenerationBias, mediumProperties):
    """I3CLSimModuleHelper::makeCherenkovWavelengthGenerator (ModuleHelper.cxx:175-263)."""
    y = np.zeros(len(wavelengthGenerationBias.values), dtype=np.float64)
    first, spacing = C.c_double(), C.c_double()
    desc = wavelengthGenerationBias._desc()
    _check(_lib.load().clsimhip_make_cherenkov_wlen_generator(C.byref(desc), mediumProperties._h, _dp(y),
                                                               C.byref(first), C.byref(spacing)))
    return I3CLSimRandomValueInterpolatedDistribution(first.value, spacing.value, y)


def makeWavelengthGenerator(unbiasedSpectrum, wavelengthGenerationBias, mediumProperties):
    """I3CLSimModuleHelper::makeWavelengthGenerator (ModuleHelper.cxx:73-171): a delta peak becomes a constant, a tabulated
    spectrum an InterpolatedDistribution on the table's own binning with the bias folded in."""
    n = max(len(getattr(unbiasedSpectrum, "values", ())), 1)
    x = np.zeros(n, dtype=np.float64)
    y = np.zeros(n, dtype=np.float64)
    out = _lib.RandomValue()
    spectrum, bias = unbiasedSpectrum._desc(), wavelengthGenerationBias._desc()
    _check(_lib.load().clsimhip_make_wlen_generator(C.byref(spectrum), C.byref(bias), mediumProperties._h, C.byref(out), _dp(x), _dp(y), n))
    if out.kind == 1:
        return I3CLSimRandomValueConstant(out.value)
    if out.kind == 3:
        return I3CLSimRandomValueInterpolatedDistribution(x[:out.n].copy(), y[:out.n].copy())
    return I3CLSimRandomValueInterpolatedDistribution(out.first, out.spacing, y[:out.n].copy())


FLASHER_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "flasher_data")
_FLASHER_LED_SPECTRA = {
    # python/GetIceCubeFlasherSpectrum.py:38-60: file under resources/flasher_data/, normalisation constant
    "LED340nm": ("flasher_led_340nm_emission_spectrum_cw_measured_20mA_pulseCurrent.txt", 24.306508),
    "LED370nm": ("flasher_led_370nm_emission_spectrum_cw_measured.txt", 15.7001863),
    "LED405nm": ("flasher_led_405nm_emission_spectrum_datasheet.txt", 8541585.10324),
    "LED450nm": ("flasher_led_450nm_emission_spectrum_datasheet.txt", 21.9792812618),
    "LED505nm": ("flasher_led_505nm_emission_spectrum_cw_measured.txt", 38.1881),
}


def GetIceCubeFlasherSpectrumData(spectrumType):
    """python/GetIceCubeFlasherSpectrum.py:38-70: (wavelengths [m], values) of an LED's emission spectrum"""
    if spectrumType not in _FLASHER_LED_SPECTRA:
        raise RuntimeError("invalid spectrumType")
    name, norm = _FLASHER_LED_SPECTRA[spectrumType]
    data = np.loadtxt(os.path.join(FLASHER_DATA, name), unpack=True)
    data[0] *= NANOMETER
    data[1] /= norm
    return data


def GetIceCubeFlasherSpectrum(spectrumType="LED405nm"):
    """python/GetIceCubeFlasherSpectrum.py:72-82; spectrumType: 'LED340nm' ... 'LED505nm', 'SC1', 'SC2'
    (I3CLSimFlasherPulse::FlasherPulseType)"""
    if spectrumType in ("SC1", "SC2"):
        return I3CLSimFunctionDeltaPeak(337.0 * NANOMETER)
    data = GetIceCubeFlasherSpectrumData(spectrumType)
    return I3CLSimFunctionFromTable(data[0], data[1])


def mwc_multipliers(count):
    a = np.zeros(count, dtype=np.uint32)
    _check(_lib.load().clsimhip_mwc_multipliers(a.ctypes.data_as(C.c_void_p), count))
    return a


def seed_streams(a, seed=12345):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    x = np.zeros(len(a), dtype=np.uint64)
    _check(_lib.load().clsimhip_seed_streams(a.ctypes.data_as(C.c_void_p), len(a), seed, x.ctypes.data_as(C.c_void_p)))
    return x


class I3CLSimSimpleGeometry:
    """public/clsim/I3CLSimSimpleGeometry.h: parallel per-DOM arrays."""

    def __init__(self, string_ids, dom_ids, x, y, z, subdetectors, om_radius):
        self.string_ids = np.ascontiguousarray(string_ids, dtype=np.int32)
        self.dom_ids = np.ascontiguousarray(dom_ids, dtype=np.uint32)
        self.x = np.ascontiguousarray(x, dtype=np.float64)
        self.y = np.ascontiguousarray(y, dtype=np.float64)
        self.z = np.ascontiguousarray(z, dtype=np.float64)
        self.subdetectors = [str(s) for s in subdetectors]
        self.om_radius = float(om_radius)

    @classmethod
    def from_text_file(cls, OMRadius, filename, ignoreStringIDsSmallerThan=1, ignoreStringIDsLargerThan=2 ** 31 - 1,
                       ignoreDomIDsSmallerThan=1, ignoreDomIDsLargerThan=60):
        """I3CLSimSimpleGeometryTextFile (private/clsim/I3CLSimSimpleGeometryTextFile.cxx:43-100); parsing happens in
        the library when the geometry is set (clsimhip_set_geometry_from_text_file)."""
        g = cls([], [], [], [], [], [], OMRadius)
        g.text_file = (str(filename), int(ignoreStringIDsSmallerThan), int(ignoreStringIDsLargerThan),
                       int(ignoreDomIDsSmallerThan), int(ignoreDomIDsLargerThan))
        return g

    @classmethod
    def from_dict(cls, g):
        return cls(g["string_ids"], g["dom_ids"], g["x"], g["y"], g["z"], g["subdetectors"], g["om_radius"])


# clsimhip_mcpe: I3MCPE(particle, npe = 1, time) with the DOM it belongs to; `id` is the step's / photon's identifier
MCPE_DTYPE = np.dtype([("id", "<u4"), ("stringID", "<i2"), ("omID", "<u2"), ("time", "<f8")])
MCPE_CONDITIONS = ("negative_weight", "off_surface", "unknown_dom", "probability_above_one")
# MCPE series (include/clsimhip.h): one entry of the particle cache, one masked module of one frame, one series of the result
MCPE_PARTICLE_DTYPE = np.dtype([("id", "<u4"), ("frame", "<u4"), ("timeShift", "<f8")])
MCPE_MASK_DTYPE = np.dtype([("frame", "<u4"), ("stringID", "<i2"), ("omID", "<u2")])
MCPE_SERIES_DTYPE = np.dtype([("frame", "<u4"), ("stringID", "<i2"), ("omID", "<u2"), ("first", "<u4"), ("count", "<u4")])
MCPE_SERIES_COUNTERS = ("unknown_particle", "masked", "unknown_dom")
# MCPE merging (include/clsimhip.h): one merged record, one entry of the flattened particle-ID map, one series' entries of it
MCPE_MERGED_DTYPE = np.dtype([("npe", "<u4"), ("stringID", "<i2"), ("omID", "<u2"), ("time", "<f8")])
MCPE_PARENT_DTYPE = np.dtype([("id", "<u4"), ("index", "<u4")])
MCPE_PARENT_RANGE_DTYPE = np.dtype([("first", "<u4"), ("count", "<u4")])


def _series_inputs(particles, masked):
    """(particles array or None, pointer, n, masked array, pointer, n) as the C ABI takes them; particles=None: no table"""
    if particles is not None:
        particles = np.ascontiguousarray(particles, dtype=MCPE_PARTICLE_DTYPE)
    masked = np.ascontiguousarray(masked if masked is not None else [], dtype=MCPE_MASK_DTYPE)
    # (an empty table is still a table: it gets an address of its own)
    keep = np.zeros(1, dtype=MCPE_PARTICLE_DTYPE) if particles is not None and len(particles) == 0 else particles
    pp = C.c_void_p(keep.ctypes.data) if keep is not None else C.c_void_p()
    return keep, pp, (len(particles) if particles is not None else 0), masked, C.c_void_p(masked.ctypes.data if len(masked) else None), len(masked)


class MCPEGenerator:
    """Detected photons -> MCPEs (clsimhip_mcpe_generator): I3CLSimPhotonToMCPEConverterForDOMs::Convert
    (private/clsim/dom/I3PhotonToMCPEConverter.cxx:602-669) as a function of the record and a seed.

    wavelengthAcceptances: up to 8 I3CLSimFunctionFromTable (equal spacing) / I3CLSimFunctionConstant; stringIDs, omIDs,
    classIndex: the class of every DOM; angularAcceptance: an I3CLSimFunctionPolynomial.  Give it to initializeHIP(...,
    mcpeGenerator=...) to run on the GPU behind the propagator, or call ConvertHost / ConvertDevice on records."""

    def __init__(self, wavelengthAcceptances, stringIDs, omIDs, classIndex, angularAcceptance, domRadius=0.16510,
                 oversizeFactor=1.0, pancakeFactor=1.0, seed=0):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self._keep = list(wavelengthAcceptances)
        descs = (_lib.Function * len(self._keep))(*[f._desc() for f in self._keep])
        sid = np.ascontiguousarray(stringIDs, dtype=np.int32)
        did = np.ascontiguousarray(omIDs, dtype=np.uint32)
        cls = np.ascontiguousarray(classIndex, dtype=np.int32)
        if not (len(sid) == len(did) == len(cls)):
            raise ValueError("stringIDs, omIDs and classIndex must have the same length")
        poly = _lib.Polynomial()
        coeff = np.ascontiguousarray(angularAcceptance.coefficients, dtype=np.float64)
        poly.n = len(coeff)
        poly.coefficients = _dp(coeff)
        poly.range_min, poly.range_max = angularAcceptance.rangemin, angularAcceptance.rangemax
        poly.underflow, poly.overflow = angularAcceptance.underflow, angularAcceptance.overflow
        _check(self._lib.clsimhip_mcpe_generator_create(descs, len(self._keep), len(sid), sid.ctypes.data_as(C.c_void_p),
                                                        did.ctypes.data_as(C.c_void_p), cls.ctypes.data_as(C.c_void_p), C.byref(poly),
                                                        float(domRadius), float(oversizeFactor), float(pancakeFactor), int(seed),
                                                        C.byref(self._h)))

    def __del__(self):
        try:
            if self._h:
                self._lib.clsimhip_mcpe_generator_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def ConvertHost(self, photons):
        """(mcpes, counters): the host twin, in input order; counters = {condition: count} (MCPE_CONDITIONS)"""
        photons = np.ascontiguousarray(photons, dtype=PHOTON_DTYPE)
        out = np.zeros(len(photons), dtype=MCPE_DTYPE)
        n, counters = C.c_size_t(), np.zeros(4, dtype=np.uint64)
        _check(self._lib.clsimhip_mcpe_convert_host(self._h, photons.ctypes.data_as(C.c_void_p), len(photons), out.ctypes.data_as(C.c_void_p),
                                                    len(out), C.byref(n), counters.ctypes.data_as(C.c_void_p)))
        return out[:n.value], dict(zip(MCPE_CONDITIONS, (int(c) for c in counters)))

    def ConvertDevice(self, d_photons, d_hit_count, capacity, d_mcpes, mcpe_capacity, d_counters, device=0, stream=0):
        """the kernel on device-resident records (addresses); d_counters: five uint32, [0] MCPEs made, [1..4] MCPE_CONDITIONS"""
        _check(self._lib.clsimhip_mcpe_convert_device(self._h, int(device), C.c_void_p(d_photons), C.c_void_p(d_hit_count), int(capacity),
                                                      C.c_void_p(d_mcpes), int(mcpe_capacity), C.c_void_p(d_counters), C.c_void_p(stream)))

    def MakeSeriesHost(self, mcpes, particles=None, masked=None):
        """(records, series, counters): the host twin of the MCPE series stage.  mcpes: MCPE_DTYPE; particles: MCPE_PARTICLE_DTYPE,
        strictly increasing in `id`, or None (every identifier is frame 0 with shift 0); masked: MCPE_MASK_DTYPE or None.  records:
        the kept MCPEs with shifted times, ascending in (frame, stringID, omID, time key, id); series: MCPE_SERIES_DTYPE, one entry per
        non-empty (frame, DOM); counters = {name: count} (MCPE_SERIES_COUNTERS)"""
        mcpes = np.ascontiguousarray(mcpes, dtype=MCPE_DTYPE)
        keep, pp, n_p, masked, mp, n_m = _series_inputs(particles, masked)
        out = np.zeros(len(mcpes), dtype=MCPE_DTYPE)
        series = np.zeros(len(mcpes), dtype=MCPE_SERIES_DTYPE)
        n_kept, n_series, counters = C.c_size_t(), C.c_size_t(), np.zeros(3, dtype=np.uint64)
        _check(self._lib.clsimhip_mcpe_series_host(self._h, mcpes.ctypes.data_as(C.c_void_p), len(mcpes), pp, n_p, mp, n_m,
                                                   out.ctypes.data_as(C.c_void_p), series.ctypes.data_as(C.c_void_p), C.byref(n_kept),
                                                   C.byref(n_series), counters.ctypes.data_as(C.c_void_p)))
        return out[:n_kept.value], series[:n_series.value], dict(zip(MCPE_SERIES_COUNTERS, (int(c) for c in counters)))

    @staticmethod
    def SeriesWorkspaceBytes(capacity, n_particles=0, n_masked=0):
        return int(_lib.load().clsimhip_mcpe_series_workspace_bytes(int(capacity), int(n_particles), int(n_masked)))

    def MakeSeriesDevice(self, d_mcpes, d_count, capacity, d_out, d_series, d_counts, d_workspace, workspace_bytes, particles=None, masked=None,
                         device=0, stream=0):
        """the kernels on device-resident MCPEs (addresses): min(*d_count, capacity) records; d_out / d_series: `capacity` entries,
        d_counts: five uint32 (kept, series, then MCPE_SERIES_COUNTERS), d_workspace: SeriesWorkspaceBytes(capacity, len(particles),
        len(masked)) bytes.  particles / masked are host arrays as for MakeSeriesHost."""
        keep, pp, n_p, masked, mp, n_m = _series_inputs(particles, masked)
        _check(self._lib.clsimhip_mcpe_series_device(self._h, int(device), C.c_void_p(d_mcpes), C.c_void_p(d_count), int(capacity), pp, n_p, mp, n_m,
                                                     C.c_void_p(d_out), C.c_void_p(d_series), C.c_void_p(d_counts), C.c_void_p(d_workspace),
                                                     int(workspace_bytes), C.c_void_p(stream)))

    @staticmethod
    def MergeHost(records, series, window):
        """(merged, merged_series, parents, parent_ranges): the host twin of the MCPE merging stage on the output of the series stage.
        records: MCPE_DTYPE, series: MCPE_SERIES_DTYPE (they partition the records), window: 0 <= window < inf.  merged:
        MCPE_MERGED_DTYPE, one per group; merged_series: the series table over the merged records; parents: MCPE_PARENT_DTYPE, the
        distinct (id, group within the series) pairs ascending in (series, id, index); parent_ranges: MCPE_PARENT_RANGE_DTYPE, one
        per series."""
        records = np.ascontiguousarray(records, dtype=MCPE_DTYPE)
        series = np.ascontiguousarray(series, dtype=MCPE_SERIES_DTYPE)
        merged, parents = np.zeros(len(records), dtype=MCPE_MERGED_DTYPE), np.zeros(len(records), dtype=MCPE_PARENT_DTYPE)
        out_series, ranges = np.zeros(len(series), dtype=MCPE_SERIES_DTYPE), np.zeros(len(series), dtype=MCPE_PARENT_RANGE_DTYPE)
        n_merged, n_parents = C.c_size_t(), C.c_size_t()
        _check(_lib.load().clsimhip_mcpe_merge_host(records.ctypes.data_as(C.c_void_p), len(records), series.ctypes.data_as(C.c_void_p), len(series),
                                                    float(window), merged.ctypes.data_as(C.c_void_p), out_series.ctypes.data_as(C.c_void_p),
                                                    parents.ctypes.data_as(C.c_void_p), ranges.ctypes.data_as(C.c_void_p), C.byref(n_merged),
                                                    C.byref(n_parents)))
        return merged[:n_merged.value], out_series, parents[:n_parents.value], ranges

    @staticmethod
    def MergeWorkspaceBytes(capacity):
        return int(_lib.load().clsimhip_mcpe_merge_workspace_bytes(int(capacity)))

    def MergeDevice(self, d_records, d_series, d_series_counts, capacity, window, d_merged, d_merged_series, d_parents, d_ranges, d_counts,
                    d_workspace, workspace_bytes, device=0, stream=0):
        """the kernels on device-resident series (addresses; pairs with MakeSeriesDevice: its d_out, d_series and d_counts); the four
        outputs hold `capacity` entries each, d_counts: two uint32 (merged records, parent entries), d_workspace:
        MergeWorkspaceBytes(capacity) bytes"""
        _check(self._lib.clsimhip_mcpe_merge_device(self._h, int(device), C.c_void_p(d_records), C.c_void_p(d_series), C.c_void_p(d_series_counts),
                                                    int(capacity), float(window), C.c_void_p(d_merged), C.c_void_p(d_merged_series),
                                                    C.c_void_p(d_parents), C.c_void_p(d_ranges), C.c_void_p(d_counts), C.c_void_p(d_workspace),
                                                    int(workspace_bytes), C.c_void_p(stream)))

    # ---- MCPE frame store (include/clsimhip.h): union and split of series forms ----
    @staticmethod
    def UnionHost(a_records, a_series, b_records, b_series, capacity=None):
        """(records, series): the host twin of the union of two series forms (MCPE_DTYPE records with their MCPE_SERIES_DTYPE table, as
        MakeSeriesHost returns them); capacity: of the output, len(a) + len(b) by default"""
        a_records, b_records = (np.ascontiguousarray(r, dtype=MCPE_DTYPE) for r in (a_records, b_records))
        a_series, b_series = (np.ascontiguousarray(s, dtype=MCPE_SERIES_DTYPE) for s in (a_series, b_series))
        capacity = len(a_records) + len(b_records) if capacity is None else int(capacity)
        out, series = np.zeros(capacity, dtype=MCPE_DTYPE), np.zeros(capacity, dtype=MCPE_SERIES_DTYPE)
        n, n_series = C.c_size_t(), C.c_size_t()
        _check(_lib.load().clsimhip_mcpe_series_union_host(a_records.ctypes.data_as(C.c_void_p), len(a_records), a_series.ctypes.data_as(C.c_void_p), len(a_series),
                                                           b_records.ctypes.data_as(C.c_void_p), len(b_records), b_series.ctypes.data_as(C.c_void_p), len(b_series),
                                                           out.ctypes.data_as(C.c_void_p), series.ctypes.data_as(C.c_void_p), capacity, C.byref(n), C.byref(n_series)))
        return out[:n.value], series[:n_series.value]

    @staticmethod
    def SplitHost(records, series, last_frame, head_capacity=None, tail_capacity=None):
        """(head_records, head_series, tail_records, tail_series): the host twin of the split -- the head holds the frames <= last_frame"""
        records = np.ascontiguousarray(records, dtype=MCPE_DTYPE)
        series = np.ascontiguousarray(series, dtype=MCPE_SERIES_DTYPE)
        head_capacity = len(records) if head_capacity is None else int(head_capacity)
        tail_capacity = len(records) if tail_capacity is None else int(tail_capacity)
        head, head_series = np.zeros(head_capacity, dtype=MCPE_DTYPE), np.zeros(head_capacity, dtype=MCPE_SERIES_DTYPE)
        tail, tail_series = np.zeros(tail_capacity, dtype=MCPE_DTYPE), np.zeros(tail_capacity, dtype=MCPE_SERIES_DTYPE)
        sizes = [C.c_size_t() for _ in range(4)]
        _check(_lib.load().clsimhip_mcpe_series_split_host(records.ctypes.data_as(C.c_void_p), len(records), series.ctypes.data_as(C.c_void_p), len(series),
                                                           int(last_frame), head.ctypes.data_as(C.c_void_p), head_series.ctypes.data_as(C.c_void_p), head_capacity,
                                                           C.byref(sizes[0]), C.byref(sizes[1]), tail.ctypes.data_as(C.c_void_p),
                                                           tail_series.ctypes.data_as(C.c_void_p), tail_capacity, C.byref(sizes[2]), C.byref(sizes[3])))
        return head[:sizes[0].value], head_series[:sizes[1].value], tail[:sizes[2].value], tail_series[:sizes[3].value]

    @staticmethod
    def UnionWorkspaceBytes(capacity_a, capacity_b):
        return int(_lib.load().clsimhip_mcpe_series_union_workspace_bytes(int(capacity_a), int(capacity_b)))

    @staticmethod
    def UnionDevice(d_a_records, d_a_series, d_a_counts, capacity_a, d_b_records, d_b_series, d_b_counts, capacity_b, d_out_records, d_out_series,
                    d_out_counts, out_capacity, d_workspace, workspace_bytes, device=0, stream=0):
        """the kernels on device-resident series forms (addresses; each input pairs with MakeSeriesDevice's d_out, d_series and d_counts,
        or with another union's output); d_out_counts: five uint32 (MCPE_UNION_COUNTS), d_workspace: UnionWorkspaceBytes(capacity_a,
        capacity_b) bytes"""
        _check(_lib.load().clsimhip_mcpe_series_union_device(int(device), C.c_void_p(d_a_records), C.c_void_p(d_a_series), C.c_void_p(d_a_counts), int(capacity_a),
                                                             C.c_void_p(d_b_records), C.c_void_p(d_b_series), C.c_void_p(d_b_counts), int(capacity_b),
                                                             C.c_void_p(d_out_records), C.c_void_p(d_out_series), C.c_void_p(d_out_counts), int(out_capacity),
                                                             C.c_void_p(d_workspace), int(workspace_bytes), C.c_void_p(stream)))

    @staticmethod
    def SplitDevice(d_records, d_series, d_counts, capacity, last_frame, d_head_records, d_head_series, d_head_counts, head_capacity, d_tail_records,
                    d_tail_series, d_tail_counts, tail_capacity, device=0, stream=0):
        """the split on device-resident series (addresses); d_head_counts / d_tail_counts: five uint32 each (records, series, 0, 0, overflow)"""
        _check(_lib.load().clsimhip_mcpe_series_split_device(int(device), C.c_void_p(d_records), C.c_void_p(d_series), C.c_void_p(d_counts), int(capacity),
                                                             int(last_frame), C.c_void_p(d_head_records), C.c_void_p(d_head_series), C.c_void_p(d_head_counts),
                                                             int(head_capacity), C.c_void_p(d_tail_records), C.c_void_p(d_tail_series), C.c_void_p(d_tail_counts),
                                                             int(tail_capacity), C.c_void_p(stream)))


# MCPE frame store (include/clsimhip.h): the five output counts of a union on the device
MCPE_UNION_COUNTS = ("records", "series", "malformed_a", "malformed_b", "overflow")
ALL_FRAMES = 0xFFFFFFFF


class MCPEFrameStore:
    """The series of several bunches accumulate per frame; finished frames leave (clsimhip_mcpe_frame_store).  device=None: a host
    store, which needs no GPU; device=k: the state lives in HBM of GPU k.  Call Add (or AddDevice) per result and Drain with the last
    frame no bunch in flight can still touch."""

    def __init__(self, capacity, device=None):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.capacity, self.device = int(capacity), device
        _check(self._lib.clsimhip_mcpe_frame_store_create(-1 if device is None else int(device), self.capacity, C.byref(self._h)))

    def __del__(self):
        try:
            if self._h:
                self._lib.clsimhip_mcpe_frame_store_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def Add(self, records, series):
        """one bunch in host memory, a series form (MakeSeriesHost's records and series, or a result's mcpes and series)"""
        records = np.ascontiguousarray(records, dtype=MCPE_DTYPE)
        series = np.ascontiguousarray(series, dtype=MCPE_SERIES_DTYPE)
        _check(self._lib.clsimhip_mcpe_frame_store_add_host(self._h, records.ctypes.data_as(C.c_void_p), len(records), series.ctypes.data_as(C.c_void_p), len(series)))

    def AddDevice(self, d_records, d_series, d_series_counts, capacity, stream=0):
        """one bunch in HBM (addresses: MakeSeriesDevice's d_out, d_series and d_counts); asynchronous on `stream`"""
        _check(self._lib.clsimhip_mcpe_frame_store_add_device(self._h, C.c_void_p(d_records), C.c_void_p(d_series), C.c_void_p(d_series_counts), int(capacity),
                                                              C.c_void_p(stream)))

    def Size(self, last_frame=ALL_FRAMES):
        """(records, series) a Drain up to last_frame would take; waits"""
        n, n_series = C.c_size_t(), C.c_size_t()
        _check(self._lib.clsimhip_mcpe_frame_store_size(self._h, int(last_frame), C.byref(n), C.byref(n_series)))
        return n.value, n_series.value

    def Drain(self, last_frame=ALL_FRAMES):
        """(records, series) of the frames <= last_frame, which leave the store; waits"""
        n, n_series = self.Size(last_frame)
        records, series = np.zeros(n, dtype=MCPE_DTYPE), np.zeros(n_series, dtype=MCPE_SERIES_DTYPE)
        got, got_series = C.c_size_t(), C.c_size_t()
        _check(self._lib.clsimhip_mcpe_frame_store_drain_host(self._h, int(last_frame), records.ctypes.data_as(C.c_void_p), series.ctypes.data_as(C.c_void_p),
                                                              n, C.byref(got), C.byref(got_series)))
        return records[:got.value], series[:got_series.value]

    def DrainDevice(self, last_frame, d_records, d_series, d_counts, capacity, stream=0):
        """the frames <= last_frame move to the caller's device buffers (addresses; d_counts: five uint32, records and series first);
        asynchronous on `stream`"""
        _check(self._lib.clsimhip_mcpe_frame_store_drain_device(self._h, int(last_frame), C.c_void_p(d_records), C.c_void_p(d_series), C.c_void_p(d_counts),
                                                                int(capacity), C.c_void_p(stream)))

    def DrainMerged(self, last_frame, window, generator=None):
        """(merged, merged_series, parents, parent_ranges) of the frames <= last_frame, as MCPEGenerator.MergeHost returns them.  A host
        store: Drain -> MergeHost; a device store: DrainDevice -> generator.MergeDevice (the MCPEGenerator whose series these are) ->
        download"""
        if self.device is None:
            return MCPEGenerator.MergeHost(*self.Drain(last_frame), window)
        if generator is None:
            raise ValueError("DrainMerged on a device store needs the MCPEGenerator whose series these are (MergeDevice is its method)")
        import torch
        dev = torch.device("cuda", int(self.device))
        capacity = max(self.Size(last_frame)[0], 1)
        sizes = (MCPE_DTYPE.itemsize, MCPE_SERIES_DTYPE.itemsize, MCPE_MERGED_DTYPE.itemsize, MCPE_SERIES_DTYPE.itemsize, MCPE_PARENT_DTYPE.itemsize,
                 MCPE_PARENT_RANGE_DTYPE.itemsize)
        d_records, d_series, d_merged, d_merged_series, d_parents, d_ranges = (torch.zeros(capacity * s, dtype=torch.uint8, device=dev) for s in sizes)
        d_counts, d_merged_counts = torch.zeros(5, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
        ws_bytes = MCPEGenerator.MergeWorkspaceBytes(capacity)
        d_ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        self.DrainDevice(last_frame, d_records.data_ptr(), d_series.data_ptr(), d_counts.data_ptr(), capacity, stream=stream)
        generator.MergeDevice(d_records.data_ptr(), d_series.data_ptr(), d_counts.data_ptr(), capacity, window, d_merged.data_ptr(), d_merged_series.data_ptr(),
                              d_parents.data_ptr(), d_ranges.data_ptr(), d_merged_counts.data_ptr(), d_ws.data_ptr(), ws_bytes, device=int(self.device), stream=stream)
        n_series = int(d_counts.cpu().numpy()[1])
        n_merged, n_parents = (int(c) for c in d_merged_counts.cpu().numpy())
        take = lambda t, dtype, n: t.cpu().numpy()[:n * dtype.itemsize].copy().view(dtype).reshape(-1)
        return (take(d_merged, MCPE_MERGED_DTYPE, n_merged), take(d_merged_series, MCPE_SERIES_DTYPE, n_series), take(d_parents, MCPE_PARENT_DTYPE, n_parents),
                take(d_ranges, MCPE_PARENT_RANGE_DTYPE, n_series))

    def drain_relabelled(self, last_frame, relabeler, window=None, generator=None):
        """The frames <= last_frame with every slice's records under its muon's identifier: drain -> relabel (-> merge) -- on a device
        store one stream carries all of it and only the download waits.  relabeler: a SeriesRelabeler.  window=None: (records,
        series); else (merged, merged_series, parents, parent_ranges) as DrainMerged returns them, with `generator` for a device store.
        A TIE_OVERFLOW of the relabel stage raises: nothing would have been delivered."""
        if self.device is None:
            records, series, counters = relabeler.mcpe_series_host(*self.Drain(last_frame))
            if counters["tie_overflow"]:
                raise I3CLSimStepToPhotonConverter_exception("series relabel: TIE_OVERFLOW = %d, nothing is delivered" % counters["tie_overflow"])
            return (records, series) if window is None else MCPEGenerator.MergeHost(records, series, window)
        if window is not None and generator is None:
            raise ValueError("drain_relabelled with a window on a device store needs the MCPEGenerator whose series these are (MergeDevice is its method)")
        import torch
        dev = torch.device("cuda", int(self.device))
        capacity = max(self.Size(last_frame)[0], 1)
        sizes = (MCPE_DTYPE.itemsize, MCPE_SERIES_DTYPE.itemsize, MCPE_DTYPE.itemsize, MCPE_SERIES_DTYPE.itemsize, MCPE_MERGED_DTYPE.itemsize,
                 MCPE_SERIES_DTYPE.itemsize, MCPE_PARENT_DTYPE.itemsize, MCPE_PARENT_RANGE_DTYPE.itemsize)
        d_records, d_series, d_new, d_new_series, d_merged, d_merged_series, d_parents, d_ranges = (
            torch.zeros(capacity * s, dtype=torch.uint8, device=dev) for s in sizes)
        d_counts, d_new_counts, d_merged_counts = (torch.zeros(k, dtype=torch.int32, device=dev) for k in (5, 5, 2))
        ws_bytes = max(relabeler.workspace_bytes(capacity, MCPE_DTYPE.itemsize), MCPEGenerator.MergeWorkspaceBytes(capacity))
        d_ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        self.DrainDevice(last_frame, d_records.data_ptr(), d_series.data_ptr(), d_counts.data_ptr(), capacity, stream=stream)
        relabeler.mcpe_series_device(d_records.data_ptr(), d_series.data_ptr(), d_counts.data_ptr(), capacity, d_new.data_ptr(), d_new_series.data_ptr(),
                                     d_new_counts.data_ptr(), d_ws.data_ptr(), ws_bytes, device=int(self.device), stream=stream)
        if window is not None:
            generator.MergeDevice(d_new.data_ptr(), d_new_series.data_ptr(), d_new_counts.data_ptr(), capacity, window, d_merged.data_ptr(),
                                  d_merged_series.data_ptr(), d_parents.data_ptr(), d_ranges.data_ptr(), d_merged_counts.data_ptr(), d_ws.data_ptr(), ws_bytes,
                                  device=int(self.device), stream=stream)
        counts = d_new_counts.cpu().numpy().view(np.uint32)
        if counts[4]:
            raise I3CLSimStepToPhotonConverter_exception("series relabel: TIE_OVERFLOW = %d, nothing is delivered" % int(counts[4]))
        n, n_series = int(counts[0]), int(counts[1])
        take = lambda t, dtype, k: t.cpu().numpy()[:k * dtype.itemsize].copy().view(dtype).reshape(-1)
        if window is None:
            return take(d_new, MCPE_DTYPE, n), take(d_new_series, MCPE_SERIES_DTYPE, n_series)
        n_merged, n_parents = (int(c) for c in d_merged_counts.cpu().numpy())
        return (take(d_merged, MCPE_MERGED_DTYPE, n_merged), take(d_merged_series, MCPE_SERIES_DTYPE, n_series), take(d_parents, MCPE_PARENT_DTYPE, n_parents),
                take(d_ranges, MCPE_PARENT_RANGE_DTYPE, n_series))


# Multi-PMT hit generator (include/clsimhip.h): clsimhip_pmt_type, clsimhip_pmt, clsimhip_pmt_module and clsimhip_pmt_hit
PMT_TYPE_DTYPE = np.dtype([("sphereRadius", "<f8"), ("firstPMT", "<i4"), ("numPMTs", "<i4"), ("glassGelSurvival", "<i4"), ("reserved", "<i4")])
PMT_DTYPE = np.dtype([("axis", "<f8", (3,)), ("position", "<f8", (3,)), ("radius", "<f8"), ("collectionEfficiency", "<f8"),
                      ("quantumEfficiency", "<i4"), ("angularAcceptance", "<i4")])
PMT_MODULE_DTYPE = np.dtype([("stringID", "<i4"), ("omID", "<u4"), ("type", "<i4"), ("reserved", "<i4"), ("rotation", "<f8", (9,))])
PMT_HIT_DTYPE = np.dtype([("id", "<u4"), ("stringID", "<i2"), ("omID", "<u2"), ("pmt", "<u4"), ("reserved", "<u4"), ("time", "<f8")])
PMT_CONDITIONS = ("unknown_module", "probability_above_one", "off_surface")
# PMT series (include/clsimhip.h): one series of the result; the particle table and the mask are the MCPE series'
PMT_SERIES_DTYPE = np.dtype([("frame", "<u4"), ("stringID", "<i2"), ("omID", "<u2"), ("pmt", "<u4"), ("first", "<u4"), ("count", "<u4"),
                             ("reserved", "<u4")])
PMT_SERIES_COUNTERS = ("unknown_particle", "masked", "unknown_channel")
# PMT photon hits (include/clsimhip.h): the records are FRAME_PHOTON_DTYPE with an MCPE_SERIES_DTYPE table in, PMT_HIT_DTYPE with a
# PMT_SERIES_DTYPE table out
PMT_PHOTON_HIT_COUNTERS = ("uncovered", "series_mismatch", "unknown_module", "probability_above_one", "off_surface")


class PMTHitGenerator:
    """Detected photons -> hits on the PMTs of segmented modules (clsimhip_pmt_generator): FindHitPMT and the per-photon body of
    I3PhotonToMCHitConverterForMultiPMT::DAQ (private/clsim/dom/I3PhotonToMCHitConverterForMultiPMT.cxx:111-227, 297-382) as a
    function of the record and a seed.

    functions: up to 64 I3CLSimFunctionFromTable (equal spacing) / I3CLSimFunctionConstant, named by index; types (PMT_TYPE_DTYPE):
    sphere radius, the type's PMTs in `pmts` and its glass / gel survival; pmts (PMT_DTYPE): axis, position, radius, collection
    efficiency, quantum efficiency over the wavelength and angular acceptance factor over the cosine of the hit angle; modules
    (PMT_MODULE_DTYPE): type and rotation (row-major, module frame -> detector frame) of every (string ID, OM ID).  Give it to
    initializeHIP(..., pmtHitGenerator=...) to run on the GPU behind the propagator, or call ConvertHost / ConvertDevice on records."""

    def __init__(self, functions, types, pmts, modules, seed=0):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self._keep = list(functions)
        descs = (_lib.Function * max(len(self._keep), 1))(*[f._desc() for f in self._keep])
        types = np.ascontiguousarray(types, dtype=PMT_TYPE_DTYPE)
        pmts = np.ascontiguousarray(pmts, dtype=PMT_DTYPE)
        modules = np.ascontiguousarray(modules, dtype=PMT_MODULE_DTYPE)
        _check(self._lib.clsimhip_pmt_generator_create(descs, len(self._keep), types.ctypes.data_as(C.c_void_p), len(types),
                                                       pmts.ctypes.data_as(C.c_void_p), len(pmts), modules.ctypes.data_as(C.c_void_p), len(modules),
                                                       int(seed), C.byref(self._h)))

    def __del__(self):
        try:
            if self._h:
                self._lib.clsimhip_pmt_generator_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def ConvertHost(self, photons):
        """(hits, counters): the host twin, in input order; counters = {condition: count} (PMT_CONDITIONS)"""
        photons = np.ascontiguousarray(photons, dtype=PHOTON_DTYPE)
        out = np.zeros(len(photons), dtype=PMT_HIT_DTYPE)
        n, counters = C.c_size_t(), np.zeros(3, dtype=np.uint64)
        _check(self._lib.clsimhip_pmt_convert_host(self._h, photons.ctypes.data_as(C.c_void_p), len(photons), out.ctypes.data_as(C.c_void_p),
                                                   len(out), C.byref(n), counters.ctypes.data_as(C.c_void_p)))
        return out[:n.value], dict(zip(PMT_CONDITIONS, (int(c) for c in counters)))

    def ConvertDevice(self, d_photons, d_hit_count, capacity, d_hits, hit_capacity, d_counters, device=0, stream=0):
        """the kernel on device-resident records (addresses); d_counters: four uint32, [0] hits made, [1..3] PMT_CONDITIONS"""
        _check(self._lib.clsimhip_pmt_convert_device(self._h, int(device), C.c_void_p(d_photons), C.c_void_p(d_hit_count), int(capacity),
                                                     C.c_void_p(d_hits), int(hit_capacity), C.c_void_p(d_counters), C.c_void_p(stream)))

    def MakeSeriesHost(self, hits, particles=None, masked=None):
        """(records, series, counters): the host twin of the PMT series stage.  hits: PMT_HIT_DTYPE; particles: MCPE_PARTICLE_DTYPE,
        strictly increasing in `id` (None: no table -- one frame, 0, no shift); masked: MCPE_MASK_DTYPE (all PMTs of a module).
        records: the kept hits with shifted times, ascending in (frame, stringID, omID, pmt, time key, id); series:
        PMT_SERIES_DTYPE, one entry per non-empty (frame, module, PMT); counters = {name: count} (PMT_SERIES_COUNTERS)"""
        hits = np.ascontiguousarray(hits, dtype=PMT_HIT_DTYPE)
        keep, pp, n_p, masked, mp, n_m = _series_inputs(particles, masked)
        out = np.zeros(len(hits), dtype=PMT_HIT_DTYPE)
        series = np.zeros(len(hits), dtype=PMT_SERIES_DTYPE)
        n_kept, n_series, counters = C.c_size_t(), C.c_size_t(), np.zeros(3, dtype=np.uint64)
        _check(self._lib.clsimhip_pmt_series_host(self._h, hits.ctypes.data_as(C.c_void_p), len(hits), pp, n_p, mp, n_m,
                                                  out.ctypes.data_as(C.c_void_p), series.ctypes.data_as(C.c_void_p), C.byref(n_kept),
                                                  C.byref(n_series), counters.ctypes.data_as(C.c_void_p)))
        return out[:n_kept.value], series[:n_series.value], dict(zip(PMT_SERIES_COUNTERS, (int(c) for c in counters)))

    @staticmethod
    def SeriesWorkspaceBytes(capacity, n_particles=0, n_masked=0):
        return int(_lib.load().clsimhip_pmt_series_workspace_bytes(int(capacity), int(n_particles), int(n_masked)))

    def MakeSeriesDevice(self, d_hits, d_count, capacity, d_out, d_series, d_counts, d_workspace, workspace_bytes, particles=None, masked=None,
                         device=0, stream=0):
        """the kernels on device-resident hits (addresses; pairs with ConvertDevice: its d_hits and d_counters): min(*d_count,
        capacity) records; d_out / d_series: `capacity` entries, d_counts: five uint32 (kept, series, then PMT_SERIES_COUNTERS),
        d_workspace: SeriesWorkspaceBytes(capacity, len(particles), len(masked)) bytes.  particles / masked are host arrays as for
        MakeSeriesHost."""
        keep, pp, n_p, masked, mp, n_m = _series_inputs(particles, masked)
        _check(self._lib.clsimhip_pmt_series_device(self._h, int(device), C.c_void_p(d_hits), C.c_void_p(d_count), int(capacity), pp, n_p, mp, n_m,
                                                    C.c_void_p(d_out), C.c_void_p(d_series), C.c_void_p(d_counts), C.c_void_p(d_workspace),
                                                    int(workspace_bytes), C.c_void_p(stream)))

    def MakeHitsFromFramePhotonsHost(self, records, series):
        """(hits, series, counters): the host twin of the PMT photon hits stage, I3PhotonToMCHitConverterForMultiPMT on stored photons.
        records: FRAME_PHOTON_DTYPE with their series table (MCPE_SERIES_DTYPE), as the frame photons stage delivers them.  hits:
        PMT_HIT_DTYPE ascending in (input series, pmt, time key, id), the time the record's own; series: PMT_SERIES_DTYPE, one entry per
        non-empty (input series, PMT); counters = {name: count} (PMT_PHOTON_HIT_COUNTERS)"""
        records = np.ascontiguousarray(records, dtype=FRAME_PHOTON_DTYPE)
        series = np.ascontiguousarray(series, dtype=MCPE_SERIES_DTYPE)
        out = np.zeros(len(records), dtype=PMT_HIT_DTYPE)
        out_series = np.zeros(len(records), dtype=PMT_SERIES_DTYPE)
        n_kept, n_series, counters = C.c_size_t(), C.c_size_t(), np.zeros(5, dtype=np.uint64)
        _check(self._lib.clsimhip_pmt_photon_hits_host(self._h, records.ctypes.data_as(C.c_void_p), len(records), series.ctypes.data_as(C.c_void_p),
                                                       len(series), out.ctypes.data_as(C.c_void_p), out_series.ctypes.data_as(C.c_void_p),
                                                       C.byref(n_kept), C.byref(n_series), counters.ctypes.data_as(C.c_void_p)))
        return out[:n_kept.value], out_series[:n_series.value], dict(zip(PMT_PHOTON_HIT_COUNTERS, (int(c) for c in counters)))

    @staticmethod
    def PMTPhotonHitsWorkspaceBytes(capacity):
        return int(_lib.load().clsimhip_pmt_photon_hits_workspace_bytes(int(capacity)))

    def MakeHitsFromFramePhotonsDevice(self, d_records, d_series, d_in_counts, capacity, d_out, d_out_series, d_counts, d_workspace, workspace_bytes,
                                       device=0, stream=0):
        """the kernels on device-resident frame photons (addresses, 16-byte aligned; pairs with FramePhotonDoms.MakeFramePhotonsDevice:
        its d_out, d_series and d_counts): min(d_in_counts[0], capacity) records, min(d_in_counts[1], capacity) series; d_out /
        d_out_series: `capacity` entries, d_counts: seven uint32 (kept, series, then PMT_PHOTON_HIT_COUNTERS), d_workspace:
        PMTPhotonHitsWorkspaceBytes(capacity) bytes; capacity <= 2^26"""
        _check(self._lib.clsimhip_pmt_photon_hits_device(self._h, int(device), C.c_void_p(d_records), C.c_void_p(d_series), C.c_void_p(d_in_counts),
                                                         int(capacity), C.c_void_p(d_out), C.c_void_p(d_out_series), C.c_void_p(d_counts),
                                                         C.c_void_p(d_workspace), int(workspace_bytes), C.c_void_p(stream)))


# Frame photons (include/clsimhip.h): one record of the result -- an I3CompressedPhoton with the module it is filed under; the
# series table is MCPE_SERIES_DTYPE, the particle table and the mask are the MCPE series'
FRAME_PHOTON_DTYPE = np.dtype([("id", "<u4"), ("stringID", "<i2"), ("omID", "<u2"), ("time", "<f8"), ("weight", "<f4"), ("wavelength", "<f4"),
                               ("groupVelocity", "<f4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("theta", "<f4"), ("phi", "<f4")])
FRAME_PHOTON_COUNTERS = ("unknown_particle", "masked", "unknown_dom", "tie_overflow")
FRAME_PHOTON_TIE_BOUND = 2048


class FramePhotonDoms:
    """The DOM list of the frame photons stage (clsimhip_frame_photon_doms): the modules a detected photon may be filed under, as the
    client module's PropagatedPhotons map files them (private/clsim/I3CLSimClientModule.cxx:359-439).  stringIDs, omIDs: one pair per
    DOM (a pair named twice is one DOM)."""

    def __init__(self, stringIDs, omIDs):
        self._lib = _lib.load()
        sid = np.ascontiguousarray(stringIDs, dtype=np.int32)
        oid = np.ascontiguousarray(omIDs, dtype=np.uint32)
        if sid.ndim != 1 or sid.shape != oid.shape:
            raise ValueError("stringIDs and omIDs: one entry per DOM each")
        h = C.c_void_p()
        _check(self._lib.clsimhip_frame_photon_doms_create(len(sid), sid.ctypes.data_as(C.c_void_p), oid.ctypes.data_as(C.c_void_p), C.byref(h)))
        self._h = h

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.clsimhip_frame_photon_doms_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def MakeFramePhotonsHost(self, photons, particles=None, masked=None):
        """(records, series, counters): the host twin of the frame photons stage.  photons: PHOTON_DTYPE with string and OM IDs;
        particles: MCPE_PARTICLE_DTYPE, strictly increasing in `id` (None: no table -- one frame, 0, no shift); masked:
        MCPE_MASK_DTYPE.  records: FRAME_PHOTON_DTYPE, the kept photons with shifted times, ascending in (frame, stringID, omID, time
        key, id, h, the eight floats' bit patterns); series: MCPE_SERIES_DTYPE, one entry per non-empty (frame, module); counters =
        {name: count} (FRAME_PHOTON_COUNTERS).  With tie_overflow > 0 there are no records."""
        photons = np.ascontiguousarray(photons, dtype=PHOTON_DTYPE)
        keep, pp, n_p, masked, mp, n_m = _series_inputs(particles, masked)
        out = np.zeros(len(photons), dtype=FRAME_PHOTON_DTYPE)
        series = np.zeros(len(photons), dtype=MCPE_SERIES_DTYPE)
        n_kept, n_series, counters = C.c_size_t(), C.c_size_t(), np.zeros(4, dtype=np.uint64)
        _check(self._lib.clsimhip_frame_photons_host(self._h, photons.ctypes.data_as(C.c_void_p), len(photons), pp, n_p, mp, n_m,
                                                     out.ctypes.data_as(C.c_void_p), series.ctypes.data_as(C.c_void_p), C.byref(n_kept),
                                                     C.byref(n_series), counters.ctypes.data_as(C.c_void_p)))
        return out[:n_kept.value], series[:n_series.value], dict(zip(FRAME_PHOTON_COUNTERS, (int(c) for c in counters)))

    @staticmethod
    def WorkspaceBytes(capacity, n_particles=0, n_masked=0):
        return int(_lib.load().clsimhip_frame_photons_workspace_bytes(int(capacity), int(n_particles), int(n_masked)))

    def MakeFramePhotonsDevice(self, d_photons, d_count, capacity, d_out, d_series, d_counts, d_workspace, workspace_bytes, particles=None, masked=None,
                               device=0, stream=0):
        """the kernels on device-resident photon records (addresses, 16-byte aligned): min(*d_count, capacity) records; d_out /
        d_series: `capacity` entries, d_counts: six uint32 (kept, series, then FRAME_PHOTON_COUNTERS), d_workspace:
        WorkspaceBytes(capacity, len(particles), len(masked)) bytes.  particles / masked are host arrays as for MakeFramePhotonsHost."""
        keep, pp, n_p, masked, mp, n_m = _series_inputs(particles, masked)
        _check(self._lib.clsimhip_frame_photons_device(self._h, int(device), C.c_void_p(d_photons), C.c_void_p(d_count), int(capacity), pp, n_p, mp, n_m,
                                                       C.c_void_p(d_out), C.c_void_p(d_series), C.c_void_p(d_counts), C.c_void_p(d_workspace),
                                                       int(workspace_bytes), C.c_void_p(stream)))


# Photon hits (include/clsimhip.h): one DOM of the maker's table; the records are FRAME_PHOTON_DTYPE in and MCPE_DTYPE out, the
# series tables MCPE_SERIES_DTYPE
PHOTON_HIT_DOM_DTYPE = np.dtype([("stringID", "<i4"), ("omID", "<u4"), ("classIndex", "<i4"), ("flags", "<u4"), ("relativeDOMEff", "<f8"),
                                 ("speCompensationFactor", "<f8"), ("dir", "<f8", (3,))])
PHOTON_HIT_HAS_STATUS, PHOTON_HIT_IN_CALIBRATION = 1, 2
PHOTON_HIT_COUNTERS = ("uncovered", "series_mismatch", "unknown_dom", "inactive", "negative_weight", "off_surface", "probability_above_one")


class PhotonHitMaker:
    """Stored frame photons -> per-frame, per-DOM time-sorted MCPEs (clsimhip_photon_hit_maker): the older I3PhotonToMCPEConverter
    (private/clsim/dom/I3PhotonToMCPEConverter.cxx:257-539) with its calibration look-ups, as a function of the records, their series
    table and a seed -- the second step of I3CLSimMakeHitsFromPhotons.

    wavelengthAcceptances, angularAcceptance: as for MCPEGenerator; doms: PHOTON_HIT_DOM_DTYPE (flags: PHOTON_HIT_HAS_STATUS,
    PHOTON_HIT_IN_CALIBRATION); the other parameters carry the module's names."""

    def __init__(self, wavelengthAcceptances, angularAcceptance, doms, DOMRadiusWithoutOversize=0.16510, DOMOversizeFactor=1.0,
                 DOMPancakeFactor=1.0, DefaultRelativeDOMEfficiency=1.0, ReplaceRelativeDOMEfficiencyWithDefault=False,
                 IgnoreDOMsWithoutDetectorStatusEntry=False, OnlyWarnAboutInvalidPhotonPositions=False, seed=0):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self._keep = list(wavelengthAcceptances)
        descs = (_lib.Function * max(len(self._keep), 1))(*[f._desc() for f in self._keep])
        doms = np.ascontiguousarray(doms, dtype=PHOTON_HIT_DOM_DTYPE)
        poly = _lib.Polynomial()
        coeff = np.ascontiguousarray(angularAcceptance.coefficients, dtype=np.float64)
        poly.n = len(coeff)
        poly.coefficients = _dp(coeff)
        poly.range_min, poly.range_max = angularAcceptance.rangemin, angularAcceptance.rangemax
        poly.underflow, poly.overflow = angularAcceptance.underflow, angularAcceptance.overflow
        cfg = _lib.PhotonHitConfig(float(DOMRadiusWithoutOversize), float(DOMOversizeFactor), float(DOMPancakeFactor),
                                   float(DefaultRelativeDOMEfficiency), int(bool(ReplaceRelativeDOMEfficiencyWithDefault)),
                                   int(bool(IgnoreDOMsWithoutDetectorStatusEntry)), int(bool(OnlyWarnAboutInvalidPhotonPositions)), 0, int(seed))
        _check(self._lib.clsimhip_photon_hit_maker_create(descs, len(self._keep), C.byref(poly), C.c_void_p(doms.ctypes.data if len(doms) else None),
                                                          len(doms), C.byref(cfg), C.byref(self._h)))

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.clsimhip_photon_hit_maker_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def Efficiency(self, stringID, omID):
        """the efficiency the maker resolved for a DOM of its table"""
        out = C.c_double()
        _check(self._lib.clsimhip_photon_hit_maker_efficiency(self._h, int(stringID), int(omID), C.byref(out)))
        return out.value

    def MakeHitsHost(self, records, series):
        """(mcpes, series, counters): the host twin.  records: FRAME_PHOTON_DTYPE with their series table (MCPE_SERIES_DTYPE), as the
        frame photons stage delivers them.  mcpes: MCPE_DTYPE ascending in (input series, time key, id); series: MCPE_SERIES_DTYPE, one
        entry per input entry that kept a record; counters = {name: count} (PHOTON_HIT_COUNTERS)"""
        records = np.ascontiguousarray(records, dtype=FRAME_PHOTON_DTYPE)
        series = np.ascontiguousarray(series, dtype=MCPE_SERIES_DTYPE)
        out = np.zeros(len(records), dtype=MCPE_DTYPE)
        out_series = np.zeros(len(series), dtype=MCPE_SERIES_DTYPE)
        n_kept, n_series, counters = C.c_size_t(), C.c_size_t(), np.zeros(7, dtype=np.uint64)
        _check(self._lib.clsimhip_photon_hits_host(self._h, records.ctypes.data_as(C.c_void_p), len(records), series.ctypes.data_as(C.c_void_p),
                                                   len(series), out.ctypes.data_as(C.c_void_p), out_series.ctypes.data_as(C.c_void_p),
                                                   C.byref(n_kept), C.byref(n_series), counters.ctypes.data_as(C.c_void_p)))
        return out[:n_kept.value], out_series[:n_series.value], dict(zip(PHOTON_HIT_COUNTERS, (int(c) for c in counters)))

    @staticmethod
    def WorkspaceBytes(capacity):
        return int(_lib.load().clsimhip_photon_hits_workspace_bytes(int(capacity)))

    def MakeHitsDevice(self, d_records, d_series, d_in_counts, capacity, d_out, d_out_series, d_counts, d_workspace, workspace_bytes, device=0, stream=0):
        """the kernels on device-resident frame photons (addresses, 16-byte aligned; pairs with FramePhotonDoms.MakeFramePhotonsDevice:
        its d_out, d_series and d_counts): min(d_in_counts[0], capacity) records, min(d_in_counts[1], capacity) series; d_out /
        d_out_series: `capacity` entries, d_counts: nine uint32 (kept, series, then PHOTON_HIT_COUNTERS), d_workspace:
        WorkspaceBytes(capacity) bytes"""
        _check(self._lib.clsimhip_photon_hits_device(self._h, int(device), C.c_void_p(d_records), C.c_void_p(d_series), C.c_void_p(d_in_counts),
                                                     int(capacity), C.c_void_p(d_out), C.c_void_p(d_out_series), C.c_void_p(d_counts),
                                                     C.c_void_p(d_workspace), int(workspace_bytes), C.c_void_p(stream)))


# Frame photon store (include/clsimhip.h): the five output counts of a union on the device are MCPE_UNION_COUNTS
def _frame_photon_form(records, series):
    return np.ascontiguousarray(records, dtype=FRAME_PHOTON_DTYPE), np.ascontiguousarray(series, dtype=MCPE_SERIES_DTYPE)


class FramePhotonStore:
    """The frame photons of several bunches accumulate per frame; finished frames leave (clsimhip_frame_photon_store): what
    MCPEFrameStore is for MCPEs, for FRAME_PHOTON_DTYPE records with their MCPE_SERIES_DTYPE table.  device=None: a host store, which
    needs no GPU; device=k: the state lives in HBM of GPU k.  Call Add (or AddDevice) per result and Drain with the last frame no
    bunch in flight can still touch."""

    def __init__(self, capacity, device=None):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.capacity, self.device = int(capacity), device
        _check(self._lib.clsimhip_frame_photon_store_create(-1 if device is None else int(device), self.capacity, C.byref(self._h)))

    def __del__(self):
        try:
            if self._h:
                self._lib.clsimhip_frame_photon_store_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def Add(self, records, series):
        """one bunch in host memory, a series form (MakeFramePhotonsHost's records and series, or a result's frame photons)"""
        records, series = _frame_photon_form(records, series)
        _check(self._lib.clsimhip_frame_photon_store_add_host(self._h, records.ctypes.data_as(C.c_void_p), len(records), series.ctypes.data_as(C.c_void_p), len(series)))

    def AddDevice(self, d_records, d_series, d_series_counts, capacity, stream=0):
        """one bunch in HBM (addresses: MakeFramePhotonsDevice's d_out, d_series and d_counts); asynchronous on `stream`"""
        _check(self._lib.clsimhip_frame_photon_store_add_device(self._h, C.c_void_p(d_records), C.c_void_p(d_series), C.c_void_p(d_series_counts), int(capacity),
                                                                C.c_void_p(stream)))

    def Size(self, last_frame=ALL_FRAMES):
        """(records, series) a Drain up to last_frame would take; waits"""
        n, n_series = C.c_size_t(), C.c_size_t()
        _check(self._lib.clsimhip_frame_photon_store_size(self._h, int(last_frame), C.byref(n), C.byref(n_series)))
        return n.value, n_series.value

    def Drain(self, last_frame=ALL_FRAMES):
        """(records, series) of the frames <= last_frame, which leave the store; waits"""
        n, n_series = self.Size(last_frame)
        records, series = np.zeros(n, dtype=FRAME_PHOTON_DTYPE), np.zeros(n_series, dtype=MCPE_SERIES_DTYPE)
        got, got_series = C.c_size_t(), C.c_size_t()
        _check(self._lib.clsimhip_frame_photon_store_drain_host(self._h, int(last_frame), records.ctypes.data_as(C.c_void_p), series.ctypes.data_as(C.c_void_p),
                                                                n, C.byref(got), C.byref(got_series)))
        return records[:got.value], series[:got_series.value]

    def DrainDevice(self, last_frame, d_records, d_series, d_counts, capacity, stream=0):
        """the frames <= last_frame move to the caller's device buffers (addresses; d_counts: five uint32, records and series first);
        asynchronous on `stream`"""
        _check(self._lib.clsimhip_frame_photon_store_drain_device(self._h, int(last_frame), C.c_void_p(d_records), C.c_void_p(d_series), C.c_void_p(d_counts),
                                                                  int(capacity), C.c_void_p(stream)))

    def DrainHits(self, last_frame, maker):
        """the hits of the frames <= last_frame: what maker.MakeHitsHost (a PhotonHitMaker) or maker.MakeHitsFromFramePhotonsHost (a
        PMTHitGenerator) returns for them.  A host store: Drain -> the maker's host twin; a device store: DrainDevice -> the maker's
        stored-photon stage behind it on the same stream -> download"""
        pmt = isinstance(maker, PMTHitGenerator)
        if self.device is None:
            return maker.MakeHitsFromFramePhotonsHost(*self.Drain(last_frame)) if pmt else maker.MakeHitsHost(*self.Drain(last_frame))
        import torch
        dev = torch.device("cuda", int(self.device))
        capacity = max(self.Size(last_frame)[0], 1)
        hit_dtype, series_dtype, names = (PMT_HIT_DTYPE, PMT_SERIES_DTYPE, PMT_PHOTON_HIT_COUNTERS) if pmt else (MCPE_DTYPE, MCPE_SERIES_DTYPE, PHOTON_HIT_COUNTERS)
        sizes = (FRAME_PHOTON_DTYPE.itemsize, MCPE_SERIES_DTYPE.itemsize, hit_dtype.itemsize, series_dtype.itemsize)
        d_records, d_series, d_hits, d_hit_series = (torch.zeros(capacity * s, dtype=torch.uint8, device=dev) for s in sizes)
        d_counts, d_hit_counts = torch.zeros(5, dtype=torch.int32, device=dev), torch.zeros(2 + len(names), dtype=torch.int32, device=dev)
        ws_bytes = PMTHitGenerator.PMTPhotonHitsWorkspaceBytes(capacity) if pmt else PhotonHitMaker.WorkspaceBytes(capacity)
        d_ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        self.DrainDevice(last_frame, d_records.data_ptr(), d_series.data_ptr(), d_counts.data_ptr(), capacity, stream=stream)
        make = maker.MakeHitsFromFramePhotonsDevice if pmt else maker.MakeHitsDevice
        make(d_records.data_ptr(), d_series.data_ptr(), d_counts.data_ptr(), capacity, d_hits.data_ptr(), d_hit_series.data_ptr(), d_hit_counts.data_ptr(),
             d_ws.data_ptr(), ws_bytes, device=int(self.device), stream=stream)
        counts = d_hit_counts.cpu().numpy().view(np.uint32)
        take = lambda t, dtype, n: t.cpu().numpy()[:n * dtype.itemsize].copy().view(dtype).reshape(-1)
        return (take(d_hits, hit_dtype, int(counts[0])), take(d_hit_series, series_dtype, int(counts[1])), dict(zip(names, (int(c) for c in counts[2:]))))

    @staticmethod
    def UnionHost(a_records, a_series, b_records, b_series, capacity=None):
        """(records, series): the host twin of the union of two series forms of frame photons; capacity: of the output, len(a) + len(b)
        by default"""
        a_records, a_series = _frame_photon_form(a_records, a_series)
        b_records, b_series = _frame_photon_form(b_records, b_series)
        capacity = len(a_records) + len(b_records) if capacity is None else int(capacity)
        out, series = np.zeros(capacity, dtype=FRAME_PHOTON_DTYPE), np.zeros(capacity, dtype=MCPE_SERIES_DTYPE)
        n, n_series = C.c_size_t(), C.c_size_t()
        _check(_lib.load().clsimhip_frame_photons_union_host(a_records.ctypes.data_as(C.c_void_p), len(a_records), a_series.ctypes.data_as(C.c_void_p), len(a_series),
                                                             b_records.ctypes.data_as(C.c_void_p), len(b_records), b_series.ctypes.data_as(C.c_void_p), len(b_series),
                                                             out.ctypes.data_as(C.c_void_p), series.ctypes.data_as(C.c_void_p), capacity, C.byref(n), C.byref(n_series)))
        return out[:n.value], series[:n_series.value]

    @staticmethod
    def SplitHost(records, series, last_frame, head_capacity=None, tail_capacity=None):
        """(head_records, head_series, tail_records, tail_series): the host twin of the split -- the head holds the frames <= last_frame"""
        records, series = _frame_photon_form(records, series)
        head_capacity = len(records) if head_capacity is None else int(head_capacity)
        tail_capacity = len(records) if tail_capacity is None else int(tail_capacity)
        head, head_series = np.zeros(head_capacity, dtype=FRAME_PHOTON_DTYPE), np.zeros(head_capacity, dtype=MCPE_SERIES_DTYPE)
        tail, tail_series = np.zeros(tail_capacity, dtype=FRAME_PHOTON_DTYPE), np.zeros(tail_capacity, dtype=MCPE_SERIES_DTYPE)
        sizes = [C.c_size_t() for _ in range(4)]
        _check(_lib.load().clsimhip_frame_photons_split_host(records.ctypes.data_as(C.c_void_p), len(records), series.ctypes.data_as(C.c_void_p), len(series),
                                                             int(last_frame), head.ctypes.data_as(C.c_void_p), head_series.ctypes.data_as(C.c_void_p), head_capacity,
                                                             C.byref(sizes[0]), C.byref(sizes[1]), tail.ctypes.data_as(C.c_void_p),
                                                             tail_series.ctypes.data_as(C.c_void_p), tail_capacity, C.byref(sizes[2]), C.byref(sizes[3])))
        return head[:sizes[0].value], head_series[:sizes[1].value], tail[:sizes[2].value], tail_series[:sizes[3].value]

    @staticmethod
    def UnionWorkspaceBytes(capacity_a, capacity_b):
        return int(_lib.load().clsimhip_frame_photons_union_workspace_bytes(int(capacity_a), int(capacity_b)))

    @staticmethod
    def UnionDevice(d_a_records, d_a_series, d_a_counts, capacity_a, d_b_records, d_b_series, d_b_counts, capacity_b, d_out_records, d_out_series,
                    d_out_counts, out_capacity, d_workspace, workspace_bytes, device=0, stream=0):
        """the kernels on device-resident series forms (addresses; each input pairs with MakeFramePhotonsDevice's d_out, d_series and
        d_counts, or with another union's output); d_out_counts: five uint32 (MCPE_UNION_COUNTS), d_workspace:
        UnionWorkspaceBytes(capacity_a, capacity_b) bytes"""
        _check(_lib.load().clsimhip_frame_photons_union_device(int(device), C.c_void_p(d_a_records), C.c_void_p(d_a_series), C.c_void_p(d_a_counts), int(capacity_a),
                                                               C.c_void_p(d_b_records), C.c_void_p(d_b_series), C.c_void_p(d_b_counts), int(capacity_b),
                                                               C.c_void_p(d_out_records), C.c_void_p(d_out_series), C.c_void_p(d_out_counts), int(out_capacity),
                                                               C.c_void_p(d_workspace), int(workspace_bytes), C.c_void_p(stream)))

    @staticmethod
    def SplitDevice(d_records, d_series, d_counts, capacity, last_frame, d_head_records, d_head_series, d_head_counts, head_capacity, d_tail_records,
                    d_tail_series, d_tail_counts, tail_capacity, device=0, stream=0):
        """the split on device-resident series (addresses); d_head_counts / d_tail_counts: five uint32 each (records, series, 0, 0, overflow)"""
        _check(_lib.load().clsimhip_frame_photons_split_device(int(device), C.c_void_p(d_records), C.c_void_p(d_series), C.c_void_p(d_counts), int(capacity),
                                                               int(last_frame), C.c_void_p(d_head_records), C.c_void_p(d_head_series), C.c_void_p(d_head_counts),
                                                               int(head_capacity), C.c_void_p(d_tail_records), C.c_void_p(d_tail_series), C.c_void_p(d_tail_counts),
                                                               int(tail_capacity), C.c_void_p(stream)))


def _pmt_hit_form(records, series):
    return np.ascontiguousarray(records, dtype=PMT_HIT_DTYPE), np.ascontiguousarray(series, dtype=PMT_SERIES_DTYPE)


class PMTHitFrameStore:
    """The PMT hit series of several bunches accumulate per frame; finished frames leave (clsimhip_pmt_hit_store): what MCPEFrameStore
    is for MCPEs and FramePhotonStore for frame photons, for PMT_HIT_DTYPE records with their PMT_SERIES_DTYPE table.  device=None: a
    host store, which needs no GPU; device=k: the state lives in HBM of GPU k.  Call Add (or AddDevice) per result and Drain with the
    last frame no bunch in flight can still touch."""

    def __init__(self, capacity, device=None):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.capacity, self.device = int(capacity), device
        _check(self._lib.clsimhip_pmt_hit_store_create(-1 if device is None else int(device), self.capacity, C.byref(self._h)))

    def __del__(self):
        try:
            if self._h:
                self._lib.clsimhip_pmt_hit_store_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def Add(self, records, series):
        """one bunch in host memory, a series form of PMT hits (MakeSeriesHost's or MakeHitsFromFramePhotonsHost's records and series,
        or a result's PMT series)"""
        records, series = _pmt_hit_form(records, series)
        _check(self._lib.clsimhip_pmt_hit_store_add_host(self._h, records.ctypes.data_as(C.c_void_p), len(records), series.ctypes.data_as(C.c_void_p), len(series)))

    def AddDevice(self, d_records, d_series, d_series_counts, capacity, stream=0):
        """one bunch in HBM (addresses: MakeSeriesDevice's or MakeHitsFromFramePhotonsDevice's d_out, d_series and d_counts);
        asynchronous on `stream`"""
        _check(self._lib.clsimhip_pmt_hit_store_add_device(self._h, C.c_void_p(d_records), C.c_void_p(d_series), C.c_void_p(d_series_counts), int(capacity),
                                                           C.c_void_p(stream)))

    def Size(self, last_frame=ALL_FRAMES):
        """(records, series) a Drain up to last_frame would take; waits"""
        n, n_series = C.c_size_t(), C.c_size_t()
        _check(self._lib.clsimhip_pmt_hit_store_size(self._h, int(last_frame), C.byref(n), C.byref(n_series)))
        return n.value, n_series.value

    def Drain(self, last_frame=ALL_FRAMES):
        """(records, series) of the frames <= last_frame, which leave the store; waits"""
        n, n_series = self.Size(last_frame)
        records, series = np.zeros(n, dtype=PMT_HIT_DTYPE), np.zeros(n_series, dtype=PMT_SERIES_DTYPE)
        got, got_series = C.c_size_t(), C.c_size_t()
        _check(self._lib.clsimhip_pmt_hit_store_drain_host(self._h, int(last_frame), records.ctypes.data_as(C.c_void_p), series.ctypes.data_as(C.c_void_p),
                                                           n, C.byref(got), C.byref(got_series)))
        return records[:got.value], series[:got_series.value]

    def DrainDevice(self, last_frame, d_records, d_series, d_counts, capacity, stream=0):
        """the frames <= last_frame move to the caller's device buffers (addresses; d_counts: five uint32, records and series first);
        asynchronous on `stream`"""
        _check(self._lib.clsimhip_pmt_hit_store_drain_device(self._h, int(last_frame), C.c_void_p(d_records), C.c_void_p(d_series), C.c_void_p(d_counts),
                                                             int(capacity), C.c_void_p(stream)))

    @staticmethod
    def UnionHost(a_records, a_series, b_records, b_series, capacity=None):
        """(records, series): the host twin of the union of two series forms of PMT hits; capacity: of the output, len(a) + len(b) by
        default"""
        a_records, a_series = _pmt_hit_form(a_records, a_series)
        b_records, b_series = _pmt_hit_form(b_records, b_series)
        capacity = len(a_records) + len(b_records) if capacity is None else int(capacity)
        out, series = np.zeros(capacity, dtype=PMT_HIT_DTYPE), np.zeros(capacity, dtype=PMT_SERIES_DTYPE)
        n, n_series = C.c_size_t(), C.c_size_t()
        _check(_lib.load().clsimhip_pmt_hits_union_host(a_records.ctypes.data_as(C.c_void_p), len(a_records), a_series.ctypes.data_as(C.c_void_p), len(a_series),
                                                        b_records.ctypes.data_as(C.c_void_p), len(b_records), b_series.ctypes.data_as(C.c_void_p), len(b_series),
                                                        out.ctypes.data_as(C.c_void_p), series.ctypes.data_as(C.c_void_p), capacity, C.byref(n), C.byref(n_series)))
        return out[:n.value], series[:n_series.value]

    @staticmethod
    def SplitHost(records, series, last_frame, head_capacity=None, tail_capacity=None):
        """(head_records, head_series, tail_records, tail_series): the host twin of the split -- the head holds the frames <= last_frame"""
        records, series = _pmt_hit_form(records, series)
        head_capacity = len(records) if head_capacity is None else int(head_capacity)
        tail_capacity = len(records) if tail_capacity is None else int(tail_capacity)
        head, head_series = np.zeros(head_capacity, dtype=PMT_HIT_DTYPE), np.zeros(head_capacity, dtype=PMT_SERIES_DTYPE)
        tail, tail_series = np.zeros(tail_capacity, dtype=PMT_HIT_DTYPE), np.zeros(tail_capacity, dtype=PMT_SERIES_DTYPE)
        sizes = [C.c_size_t() for _ in range(4)]
        _check(_lib.load().clsimhip_pmt_hits_split_host(records.ctypes.data_as(C.c_void_p), len(records), series.ctypes.data_as(C.c_void_p), len(series),
                                                        int(last_frame), head.ctypes.data_as(C.c_void_p), head_series.ctypes.data_as(C.c_void_p), head_capacity,
                                                        C.byref(sizes[0]), C.byref(sizes[1]), tail.ctypes.data_as(C.c_void_p),
                                                        tail_series.ctypes.data_as(C.c_void_p), tail_capacity, C.byref(sizes[2]), C.byref(sizes[3])))
        return head[:sizes[0].value], head_series[:sizes[1].value], tail[:sizes[2].value], tail_series[:sizes[3].value]

    @staticmethod
    def UnionWorkspaceBytes(capacity_a, capacity_b):
        return int(_lib.load().clsimhip_pmt_hits_union_workspace_bytes(int(capacity_a), int(capacity_b)))

    @staticmethod
    def UnionDevice(d_a_records, d_a_series, d_a_counts, capacity_a, d_b_records, d_b_series, d_b_counts, capacity_b, d_out_records, d_out_series,
                    d_out_counts, out_capacity, d_workspace, workspace_bytes, device=0, stream=0):
        """the kernels on device-resident series forms (addresses; each input pairs with MakeSeriesDevice's or
        MakeHitsFromFramePhotonsDevice's d_out, d_series and d_counts, or with another union's output); d_out_counts: five uint32
        (MCPE_UNION_COUNTS), d_workspace: UnionWorkspaceBytes(capacity_a, capacity_b) bytes"""
        _check(_lib.load().clsimhip_pmt_hits_union_device(int(device), C.c_void_p(d_a_records), C.c_void_p(d_a_series), C.c_void_p(d_a_counts), int(capacity_a),
                                                          C.c_void_p(d_b_records), C.c_void_p(d_b_series), C.c_void_p(d_b_counts), int(capacity_b),
                                                          C.c_void_p(d_out_records), C.c_void_p(d_out_series), C.c_void_p(d_out_counts), int(out_capacity),
                                                          C.c_void_p(d_workspace), int(workspace_bytes), C.c_void_p(stream)))

    @staticmethod
    def SplitDevice(d_records, d_series, d_counts, capacity, last_frame, d_head_records, d_head_series, d_head_counts, head_capacity, d_tail_records,
                    d_tail_series, d_tail_counts, tail_capacity, device=0, stream=0):
        """the split on device-resident series (addresses); d_head_counts / d_tail_counts: five uint32 each (records, series, 0, 0, overflow)"""
        _check(_lib.load().clsimhip_pmt_hits_split_device(int(device), C.c_void_p(d_records), C.c_void_p(d_series), C.c_void_p(d_counts), int(capacity),
                                                          int(last_frame), C.c_void_p(d_head_records), C.c_void_p(d_head_series), C.c_void_p(d_head_counts),
                                                          int(head_capacity), C.c_void_p(d_tail_records), C.c_void_p(d_tail_series), C.c_void_p(d_tail_counts),
                                                          int(tail_capacity), C.c_void_p(stream)))


class CableShadow:
    """The cylinder set of the cable shadow stage (clsimhip_cable_shadow; include/clsimhip.h: "Cable shadow"): a detected photon whose
    last `distance` metres of path meet a solid finite cylinder is shadowed.  top, bottom: [n, 3] end points; radius: [n] or one value
    for all.  At most CABLE_SHADOW_MAX_CYLINDERS cylinders."""

    def __init__(self, top, bottom, radius, distance):
        self._lib = _lib.load()
        top = np.ascontiguousarray(top, dtype=np.float64).reshape(-1, 3)
        bottom = np.ascontiguousarray(bottom, dtype=np.float64).reshape(-1, 3)
        radius = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float64), (len(top),)))
        if top.shape != bottom.shape:
            raise ValueError("top and bottom: one point per cylinder each")
        h = C.c_void_p()
        _check(self._lib.clsimhip_cable_shadow_create(len(top), top.ctypes.data_as(C.c_void_p), bottom.ctypes.data_as(C.c_void_p),
                                                      radius.ctypes.data_as(C.c_void_p), float(distance), C.byref(h)))
        self._h = h
        self.num_cylinders = len(top)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.clsimhip_cable_shadow_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def MakeHost(self, photons):
        """(flags, lit, counts): the host twin.  photons: PHOTON_DTYPE; flags: one uint8 per record, 1 = shadowed; lit: the records with
        flag 0, in input order; counts = {"tested": ..., "shadowed": ...}"""
        photons = np.ascontiguousarray(photons, dtype=PHOTON_DTYPE)
        flags = np.zeros(len(photons), dtype=np.uint8)
        lit = np.zeros(len(photons), dtype=PHOTON_DTYPE)
        n_lit, counts = C.c_size_t(), np.zeros(2, dtype=np.uint64)
        _check(self._lib.clsimhip_cable_shadow_host(self._h, photons.ctypes.data_as(C.c_void_p), len(photons), flags.ctypes.data_as(C.c_void_p),
                                                    lit.ctypes.data_as(C.c_void_p), C.byref(n_lit), counts.ctypes.data_as(C.c_void_p)))
        return flags, lit[:n_lit.value], dict(zip(CABLE_SHADOW_COUNTS, (int(c) for c in counts)))

    @staticmethod
    def WorkspaceBytes(capacity):
        return int(_lib.load().clsimhip_cable_shadow_workspace_bytes(int(capacity)))

    def MakeDevice(self, d_photons, d_count, capacity, d_flags, d_lit, d_counts, d_workspace, workspace_bytes, device=0, stream=0):
        """the kernels on device-resident photon records (addresses; d_photons, d_lit and d_workspace 16-byte aligned): min(*d_count,
        capacity) records; d_flags: `capacity` bytes, d_lit: `capacity` records, d_counts: three uint32 (lit, tested, shadowed),
        d_workspace: WorkspaceBytes(capacity) bytes"""
        _check(self._lib.clsimhip_cable_shadow_device(self._h, int(device), C.c_void_p(d_photons), C.c_void_p(d_count), int(capacity), C.c_void_p(d_flags),
                                                      C.c_void_p(d_lit), C.c_void_p(d_counts), C.c_void_p(d_workspace), int(workspace_bytes), C.c_void_p(stream)))


CABLE_SHADOW_COUNTS = ("tested", "shadowed")
CABLE_SHADOW_MAX_CYLINDERS = 16384

# Event statistics (include/clsimhip.h): one record per entry of the bunch's particle table (one without a table) -- counts, and the
# weight sums as exact integers in units of 2^-149 (six little-endian uint64 words, two's complement) with their +inf, -inf, NaN terms
EVENT_STATISTICS_DTYPE = np.dtype([("id", "<u4"), ("frame", "<u4"), ("generatedCount", "<u8"), ("atDOMsCount", "<u8"), ("generatedSum", "<u8", (6,)),
                                   ("atDOMsSum", "<u8", (6,)), ("generatedSpecial", "<u4", (3,)), ("atDOMsSpecial", "<u4", (3,))])
EVENT_STATISTICS_COUNTERS = ("unknown_particle", "masked", "unknown_step_particle")
assert EVENT_STATISTICS_DTYPE.itemsize == 144


class EventStatistics:
    """The event statistics stage on records (include/clsimhip.h: "Event statistics"): the client module's I3CLSimEventStatistics
    (private/clsim/I3CLSimClientModule.cxx:513-520, 386-405) with exact integer weight sums.  Nothing to configure: static methods."""

    @staticmethod
    def MakeHost(steps, photons, particles=None, masked=None):
        """(records, counters): the host twin.  steps: STEP_DTYPE; photons: PHOTON_DTYPE with string and OM IDs; particles:
        MCPE_PARTICLE_DTYPE, strictly increasing in `id` (None: no table -- one record, id 0 and frame 0); masked: MCPE_MASK_DTYPE.
        records: EVENT_STATISTICS_DTYPE, one per table entry in table order; counters = {name: count} (EVENT_STATISTICS_COUNTERS)"""
        steps = np.ascontiguousarray(steps if steps is not None else [], dtype=STEP_DTYPE)
        photons = np.ascontiguousarray(photons if photons is not None else [], dtype=PHOTON_DTYPE)
        keep, pp, n_p, masked, mp, n_m = _series_inputs(particles, masked)
        out = np.zeros(n_p if particles is not None else 1, dtype=EVENT_STATISTICS_DTYPE)
        counters = np.zeros(3, dtype=np.uint64)
        _check(_lib.load().clsimhip_event_statistics_host(C.c_void_p(steps.ctypes.data if len(steps) else None), len(steps),
                                                          C.c_void_p(photons.ctypes.data if len(photons) else None), len(photons), pp, n_p, mp, n_m,
                                                          C.c_void_p(out.ctypes.data if len(out) else None), counters.ctypes.data_as(C.c_void_p)))
        return out, dict(zip(EVENT_STATISTICS_COUNTERS, (int(c) for c in counters)))

    @staticmethod
    def WorkspaceBytes(n_particles=0, n_masked=0):
        return int(_lib.load().clsimhip_event_statistics_workspace_bytes(int(n_particles), int(n_masked)))

    @staticmethod
    def MakeDevice(d_steps, n_steps, d_photons, d_count, capacity, d_out, d_counters, d_workspace, workspace_bytes, particles=None, masked=None,
                   device=0, stream=0):
        """the kernels on device-resident steps and photon records (addresses): n_steps steps and min(*d_count, capacity) photons;
        d_out: one EVENT_STATISTICS_DTYPE record per table entry (one without a table), d_counters: four uint32
        (EVENT_STATISTICS_COUNTERS, then the records written), d_workspace: WorkspaceBytes(len(particles), len(masked)) bytes.
        particles / masked are host arrays as for MakeHost."""
        keep, pp, n_p, masked, mp, n_m = _series_inputs(particles, masked)
        _check(_lib.load().clsimhip_event_statistics_device(int(device), C.c_void_p(d_steps), int(n_steps), C.c_void_p(d_photons), C.c_void_p(d_count),
                                                            int(capacity), pp, n_p, mp, n_m, C.c_void_p(d_out), C.c_void_p(d_counters),
                                                            C.c_void_p(d_workspace), int(workspace_bytes), C.c_void_p(stream)))

    @staticmethod
    def Add(acc, rec):
        """acc + rec as a new record (clsimhip_event_statistics_add): sums with carry, counts, special counters; acc's id and frame"""
        out = np.array(acc, dtype=EVENT_STATISTICS_DTYPE).reshape(1).copy()
        rec = np.array(rec, dtype=EVENT_STATISTICS_DTYPE).reshape(1)
        _check(_lib.load().clsimhip_event_statistics_add(C.c_void_p(out.ctypes.data), C.c_void_p(rec.ctypes.data)))
        return out[0]

    @staticmethod
    def Weight(words, special):
        """a sum as a float (clsimhip_event_statistics_weight): rounded once to nearest-even; NaN / +-inf from the special counters"""
        words = np.ascontiguousarray(words, dtype=np.uint64).reshape(6)
        special = np.ascontiguousarray(special, dtype=np.uint32).reshape(3)
        return float(_lib.load().clsimhip_event_statistics_weight(C.c_void_p(words.ctypes.data), C.c_void_p(special.ctypes.data)))


class ConversionResult(tuple):
    """What GetConversionResult / GetConversionResultInPlace return: the tuple (identifier, photons[, histories]) / (identifier,
    photons, release), with the bunch's MCPEs (MCPE_DTYPE) as attribute `mcpes` when the converter has an MCPE generator (None
    otherwise).  With the MCPE series stage `mcpes` are the sorted records, `series` their series table (MCPE_SERIES_DTYPE) and
    `masked` the bunch's MASKED count; with the MCPE merging stage `merged` (MCPE_MERGED_DTYPE), `merged_series`, `parents`
    (MCPE_PARENT_DTYPE) and `parent_ranges` (MCPE_PARENT_RANGE_DTYPE) beside them.  With a PMT hit generator `pmt_hits` holds the bunch's hits (PMT_HIT_DTYPE);
    with the PMT series stage they are the sorted records, `pmt_series` their series table (PMT_SERIES_DTYPE) and `masked` the
    bunch's MASKED count.  With the frame photons stage `frame_photons` (FRAME_PHOTON_DTYPE), `frame_photon_series` (MCPE_SERIES_DTYPE)
    and `frame_photons_masked`.  With the cable shadow stage `shadow_flags` (one uint8 per photon record, 1 = shadowed) and
    `shadow_counts` ({"tested", "shadowed"}); the photons stay all detected photons, every other stage's records come from the lit ones."""
    shadow_flags = None
    shadow_counts = None
    frame_photons = None
    frame_photon_series = None
    frame_photons_masked = None
    mcpes = None
    series = None
    masked = None
    merged = None
    merged_series = None
    parents = None
    parent_ranges = None
    pmt_hits = None
    pmt_series = None


class I3CLSimStepToPhotonConverterHIP:
    """MI355X implementation of I3CLSimStepToPhotonConverter."""

    def __init__(self, device=0):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        _check(self._lib.clsimhip_create(int(device), C.byref(self._h)))
        self._history_entries = 0
        self._mcpe = None
        self._series = False
        self._merging = False
        self._pmt = None
        self._pmt_series = False
        self._frame_photons = False
        self._shadow = None
        self._event_statistics = False

    def __del__(self):
        try:
            if self._h:
                self._lib.clsimhip_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _call(self, name, *args):
        _check(getattr(self._lib, name)(self._h, *args), self._h)

    # ---- configuration ----
    def SetWlenGenerators(self, wlenGenerators):
        descs = (_lib.RandomValue * len(wlenGenerators))(*[g._desc() for g in wlenGenerators])
        self._call("clsimhip_set_wlen_generators", descs, len(wlenGenerators))

    def SetWlenBias(self, wlenBias):
        d = wlenBias._desc()
        self._call("clsimhip_set_wlen_bias", C.byref(d))

    def SetMediumProperties(self, mediumProperties):
        self._call("clsimhip_set_medium_properties", mediumProperties._h)

    def SetGeometry(self, geometry):
        g = geometry
        if getattr(g, "text_file", None):
            fn, smin, smax, dmin, dmax = g.text_file
            self._call("clsimhip_set_geometry_from_text_file", fn.encode(), g.om_radius, smin, smax, dmin, dmax)
            return
        names = (C.c_char_p * len(g.subdetectors))(*[s.encode() for s in g.subdetectors])
        self._call("clsimhip_set_geometry", len(g.string_ids), g.string_ids.ctypes.data_as(C.c_void_p),
                   g.dom_ids.ctypes.data_as(C.c_void_p), g.x.ctypes.data_as(C.c_void_p),
                   g.y.ctypes.data_as(C.c_void_p), g.z.ctypes.data_as(C.c_void_p), names, g.om_radius)

    def SetEnableDoubleBuffering(self, v): self._call("clsimhip_set_enable_double_buffering", int(bool(v)))
    def SetDoublePrecision(self, v): self._call("clsimhip_set_double_precision", int(bool(v)))
    def SetStopDetectedPhotons(self, v): self._call("clsimhip_set_stop_detected_photons", int(bool(v)))
    def SetSaveAllPhotons(self, v): self._call("clsimhip_set_save_all_photons", int(bool(v)))
    def SetSaveAllPhotonsPrescale(self, v): self._call("clsimhip_set_save_all_photons_prescale", float(v))
    def SetFixedNumberOfAbsorptionLengths(self, v): self._call("clsimhip_set_fixed_number_of_absorption_lengths", float(v))
    def SetDOMPancakeFactor(self, v): self._call("clsimhip_set_dom_pancake_factor", float(v))
    def SetPhotonHistoryEntries(self, v):
        self._call("clsimhip_set_photon_history_entries", int(v))
        self._history_entries = int(v)
    def SetMCPEGenerator(self, generator, keepPhotons=True):
        """generator: an MCPEGenerator or None (off).  keepPhotons=False: results carry MCPEs only, the photon records stay on
        the device (the client module's two switches, frame->photons / frame->hits)"""
        self._call("clsimhip_set_mcpe_generator", generator._h if generator is not None else None, int(bool(keepPhotons)))
        self._mcpe = generator
    def SetPMTHitGenerator(self, generator, keepPhotons=True):
        """generator: a PMTHitGenerator or None (off); keepPhotons as for SetMCPEGenerator.  Before Initialize() only; Compile()
        refuses it beside an MCPE generator."""
        self._call("clsimhip_set_pmt_generator", generator._h if generator is not None else None, int(bool(keepPhotons)))
        self._pmt = generator
    def SetMCPESeries(self, on=True):
        """the sorting stage behind the MCPE generator: every result's MCPEs come back as per-frame, per-DOM time-sorted series
        (result attributes `mcpes`, `series`, `masked`).  Before Initialize() only; Compile() refuses it without a generator."""
        self._call("clsimhip_set_mcpe_series", int(bool(on)))
        self._series = bool(on)
    def SetPMTSeries(self, on=True):
        """the sorting stage behind the PMT hit generator: every result's hits come back as per-frame, per-module, per-PMT time-sorted
        series (result attributes `pmt_hits`, `pmt_series`, `masked`).  Before Initialize() only; Compile() refuses it without a PMT
        hit generator."""
        self._call("clsimhip_set_pmt_series", int(bool(on)))
        self._pmt_series = bool(on)
    def SetFramePhotons(self, on=True, keepPhotons=True):
        """the sorting stage behind the propagation kernel's photon records: every result's detected photons come back as per-frame,
        per-module sorted series of compressed photons, the client module's PropagatedPhotons (result attributes `frame_photons`,
        `frame_photon_series`, `frame_photons_masked`); independent of the hit generators.  keepPhotons=False leaves the 80-byte
        records on the device.  Before Initialize() only."""
        self._call("clsimhip_set_frame_photons", int(bool(on)), int(bool(keepPhotons)))
        self._frame_photons = bool(on)
    def SetCableShadow(self, shadow):
        """shadow: a CableShadow or None (off, the default).  The stage runs right behind the propagation kernel; the MCPE generator, the
        PMT hit generator, their series stages and the frame photons stage then read the lit records.  Results keep all detected
        photons, with `shadow_flags` aligned to them and `shadow_counts`.  Before Initialize() only."""
        self._call("clsimhip_set_cable_shadow", shadow._h if shadow is not None else None)
        self._shadow = shadow
    def SetEventStatistics(self, on=True):
        """the counting stage over every bunch's steps and ALL its detected photons (also with a cable shadow bound): per particle of
        the bunch's table, photons generated and at DOMs as counts and exact weight sums (result attributes `event_statistics`,
        EVENT_STATISTICS_DTYPE, and `event_statistics_counters`).  Works with keepPhotons=False.  Before Initialize() only."""
        self._call("clsimhip_set_event_statistics", int(bool(on)))
        self._event_statistics = bool(on)
    def SetMCPEMerging(self, window, on=True):
        """the merging stage behind the series stage: records of a series within `window` of their group's opener become one merged
        record (result attributes `merged`, `merged_series`, `parents`, `parent_ranges`; `mcpes` and `series` stay the unmerged
        ones).  Before Initialize() only; Compile() refuses it without SetMCPESeries."""
        self._call("clsimhip_set_mcpe_merging", int(bool(on)), float(window))
        self._merging = bool(on)
    def SetWorkgroupSize(self, v): self._call("clsimhip_set_workgroup_size", int(v))
    def SetMaxNumWorkitems(self, v): self._call("clsimhip_set_max_num_workitems", int(v))

    def Compile(self): self._call("clsimhip_compile")

    def GetMaxWorkgroupSize(self):
        v = C.c_size_t()
        self._call("clsimhip_get_max_workgroup_size", C.byref(v))
        return v.value

    def Initialize(self, seed=12345):
        self._call("clsimhip_initialize", int(seed))

    def InitializeWithStreams(self, x, a):
        x = np.ascontiguousarray(x, dtype=np.uint64); a = np.ascontiguousarray(a, dtype=np.uint32)
        self._call("clsimhip_initialize_with_streams", x.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), len(x))

    def IsInitialized(self):
        return bool(self._lib.clsimhip_is_initialized(self._h))

    # ---- steady state ----
    def EnqueueSteps(self, steps, identifier, particles=None, masked=None):
        """particles (MCPE_PARTICLE_DTYPE, strictly increasing in `id`) and masked (MCPE_MASK_DTYPE): the bunch's particle table and
        ignored modules for the MCPE series stage (SetMCPESeries), the PMT series stage (SetPMTSeries), the frame photons stage
        (SetFramePhotons) or the event statistics stage (SetEventStatistics); without them the bunch is one frame, 0, with no shift"""
        if steps is None:
            raise I3CLSimStepToPhotonConverter_exception("Steps pointer is (null)!", _lib.ERR_ARGUMENT)
        steps = np.ascontiguousarray(steps, dtype=STEP_DTYPE)
        if particles is None and masked is None:
            self._call("clsimhip_enqueue_steps", steps.ctypes.data_as(C.c_void_p), len(steps), int(identifier))
            return
        keep, pp, n_p, masked, mp, n_m = _series_inputs(particles, masked)
        self._call("clsimhip_enqueue_steps_with_particles", steps.ctypes.data_as(C.c_void_p), len(steps), int(identifier), pp, n_p, mp, n_m)

    @staticmethod
    def _copy_records(address, count, dtype):
        """copy of `count` records of `dtype` at `address` (a c_void_p the library filled in)"""
        dtype = np.dtype(dtype)
        array = np.zeros(count, dtype=dtype)
        if count:
            C.memmove(array.ctypes.data, address.value, count * dtype.itemsize)
        return array

    def _result_mcpes(self, ptr):
        """copy of the MCPEs of the result `ptr` belongs to (None without a generator); with the MCPE series stage the tuple
        (sorted records, series table, MASKED count)"""
        if self._mcpe is None:
            return None
        if self._series:
            mp, mn, sp, sn, masked = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t(), C.c_uint64()
            self._call("clsimhip_get_result_mcpe_series", ptr, C.byref(mp), C.byref(mn), C.byref(sp), C.byref(sn), C.byref(masked))
            mcpes, series = self._copy_records(mp, mn.value, MCPE_DTYPE), self._copy_records(sp, sn.value, MCPE_SERIES_DTYPE)
            if self._merging:
                return mcpes, series, int(masked.value), self._result_merged(ptr)
            return mcpes, series, int(masked.value)
        mp, mn = C.c_void_p(), C.c_size_t()
        self._call("clsimhip_get_result_mcpes", ptr, C.byref(mp), C.byref(mn))
        return self._copy_records(mp, mn.value, MCPE_DTYPE)

    def _result_merged(self, ptr):
        """copies of (merged records, merged series table, parents, parent ranges) of the result `ptr` belongs to"""
        gp, gn, sp, sn, pp, pn, rp = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t(), C.c_void_p()
        self._call("clsimhip_get_result_mcpe_merged", ptr, C.byref(gp), C.byref(gn), C.byref(sp), C.byref(sn), C.byref(pp), C.byref(pn), C.byref(rp))
        return (self._copy_records(gp, gn.value, MCPE_MERGED_DTYPE), self._copy_records(sp, sn.value, MCPE_SERIES_DTYPE),
                self._copy_records(pp, pn.value, MCPE_PARENT_DTYPE), self._copy_records(rp, sn.value, MCPE_PARENT_RANGE_DTYPE))

    def _result_pmt_hits(self, ptr):
        """copy of the PMT hits of the result `ptr` belongs to (None without a PMT hit generator); with the PMT series stage the
        tuple (sorted records, series table, MASKED count)"""
        if self._pmt is None:
            return None
        if self._pmt_series:
            hp, hn, sp, sn, masked = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t(), C.c_uint64()
            self._call("clsimhip_get_result_pmt_series", ptr, C.byref(hp), C.byref(hn), C.byref(sp), C.byref(sn), C.byref(masked))
            return self._copy_records(hp, hn.value, PMT_HIT_DTYPE), self._copy_records(sp, sn.value, PMT_SERIES_DTYPE), int(masked.value)
        hp, hn = C.c_void_p(), C.c_size_t()
        self._call("clsimhip_get_result_pmt_hits", ptr, C.byref(hp), C.byref(hn))
        return self._copy_records(hp, hn.value, PMT_HIT_DTYPE)

    def _has_handle(self):
        """a result without photon records still has a handle to release when a hit maker is attached"""
        return self._mcpe is not None or self._pmt is not None or self._frame_photons or self._shadow is not None or self._event_statistics

    def GetResultEventStatistics(self, ptr):
        """copies of the event statistics of the result `ptr` belongs to: (records, {counter: count}); CLSIMHIP_ERR_STATE without
        SetEventStatistics"""
        rp, rn, counters = C.c_void_p(), C.c_size_t(), np.zeros(3, dtype=np.uint64)
        self._call("clsimhip_get_result_event_statistics", ptr, C.byref(rp), C.byref(rn), counters.ctypes.data_as(C.c_void_p))
        return self._copy_records(rp, rn.value, EVENT_STATISTICS_DTYPE), dict(zip(EVENT_STATISTICS_COUNTERS, (int(c) for c in counters)))

    def _attach_event_statistics(self, result, es):
        if es is not None:
            result.event_statistics, result.event_statistics_counters = es

    def GetResultCableShadow(self, ptr):
        """copies of the cable shadow flags of the result `ptr` belongs to and its counts: (flags, {"tested", "shadowed"});
        CLSIMHIP_ERR_STATE without SetCableShadow"""
        fp, fn, counts = C.c_void_p(), C.c_size_t(), np.zeros(2, dtype=np.uint64)
        self._call("clsimhip_get_result_cable_shadow", ptr, C.byref(fp), C.byref(fn), counts.ctypes.data_as(C.c_void_p))
        return self._copy_records(fp, fn.value, np.uint8), dict(zip(CABLE_SHADOW_COUNTS, (int(c) for c in counts)))

    def _attach_cable_shadow(self, result, shadow):
        if shadow is not None:
            result.shadow_flags, result.shadow_counts = shadow

    def GetResultFramePhotons(self, ptr):
        """copies of the frame photons of the result `ptr` belongs to: (records, series table, MASKED count); CLSIMHIP_ERR_STATE
        without SetFramePhotons"""
        rp, rn, sp, sn, masked = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t(), C.c_uint64()
        self._call("clsimhip_get_result_frame_photons", ptr, C.byref(rp), C.byref(rn), C.byref(sp), C.byref(sn), C.byref(masked))
        return self._copy_records(rp, rn.value, FRAME_PHOTON_DTYPE), self._copy_records(sp, sn.value, MCPE_SERIES_DTYPE), int(masked.value)

    def _attach_frame_photons(self, result, fp):
        if fp is not None:
            result.frame_photons, result.frame_photon_series, result.frame_photons_masked = fp

    def GetConversionResult(self, with_histories=False, out=None):
        """ConversionResult_t (I3CLSimStepToPhotonConverter.h:70-90): (identifier, photons), plus with
        with_histories=True the photonHistories as a list of [k_i, 4] arrays (k_i = min(numScatters_i,
        PhotonHistoryEntries); None when no histories are recorded).  The photons are copied out of the library's buffer
        (like the C++ adapter copies them into the I3CLSimPhotonSeries it hands to the caller): into `out`, a PHOTON_DTYPE
        array the caller recycles, when it is given and large enough -- a view of it is returned.  With an MCPE generator the
        result's attribute `mcpes` holds the bunch's MCPEs."""
        # a recycled buffer is written through its raw address: it must be exactly what the records are -- checked before a
        # result is taken, whatever that result holds (the contract does not depend on the data)
        if out is not None and not (isinstance(out, np.ndarray) and out.dtype == PHOTON_DTYPE and out.ndim == 1 and out.flags.c_contiguous
                                    and out.flags.writeable):
            raise ValueError("GetConversionResult(out=...): a writeable, C-contiguous one-dimensional array of PHOTON_DTYPE (80-byte records) is required")
        ident, ptr, n = C.c_uint32(), C.c_void_p(), C.c_size_t()
        self._call("clsimhip_get_conversion_result", C.byref(ident), C.byref(ptr), C.byref(n))
        histories = None
        try:            # whatever fails below, the result goes back to the library
            if n.value:
                buf = (C.c_char * (n.value * 80)).from_address(ptr.value)
                if out is not None and len(out) >= n.value:
                    C.memmove(out.ctypes.data, ptr.value, n.value * 80)
                    photons = out[:n.value]
                else:
                    photons = np.frombuffer(buf, dtype=PHOTON_DTYPE).copy()
                if with_histories:
                    hp, entries = C.POINTER(C.c_float)(), C.c_uint32()
                    self._call("clsimhip_get_result_histories", ptr, C.byref(hp), C.byref(entries))
                    if hp and entries.value:
                        flat = np.ctypeslib.as_array(hp, shape=(n.value, entries.value, 4)).copy()
                        histories = [flat[i, :min(int(photons["numScatters"][i]), entries.value)] for i in range(n.value)]
            else:
                photons = np.zeros(0, dtype=PHOTON_DTYPE)
                if with_histories and self._history_entries:
                    histories = []
            mcpes = self._result_mcpes(ptr)
            pmt_hits = self._result_pmt_hits(ptr)
            fp = self.GetResultFramePhotons(ptr) if self._frame_photons else None
            shadow = self.GetResultCableShadow(ptr) if self._shadow is not None else None
            es = self.GetResultEventStatistics(ptr) if self._event_statistics else None
        finally:
            if n.value or self._has_handle():
                self._call("clsimhip_release_result", ptr)
        result = ConversionResult((ident.value, photons, histories) if with_histories else (ident.value, photons))
        self._attach_mcpes(result, mcpes)
        self._attach_pmt_hits(result, pmt_hits)
        self._attach_frame_photons(result, fp)
        self._attach_cable_shadow(result, shadow)
        self._attach_event_statistics(result, es)
        return result

    def GetConversionResultInPlace(self):
        """(identifier, photons, release): `photons` is a read-only view of the library's page-locked result buffer -- what
        a C or C++ consumer that works on the records where they are gets from clsimhip_get_conversion_result -- valid until
        `release()` is called (clsimhip_release_result), which the caller must do.  With an MCPE generator the returned tuple's
        attribute `mcpes` holds a copy of the bunch's MCPEs (also when the result carries no photon records)."""
        ident, ptr, n = C.c_uint32(), C.c_void_p(), C.c_size_t()
        self._call("clsimhip_get_conversion_result", C.byref(ident), C.byref(ptr), C.byref(n))
        try:
            mcpes = self._result_mcpes(ptr)
            pmt_hits = self._result_pmt_hits(ptr)
            fp = self.GetResultFramePhotons(ptr) if self._frame_photons else None
            shadow = self.GetResultCableShadow(ptr) if self._shadow is not None else None
            es = self.GetResultEventStatistics(ptr) if self._event_statistics else None
        except Exception:
            if n.value or self._has_handle():
                self._call("clsimhip_release_result", ptr)
            raise
        if not n.value:
            if self._has_handle():              # (the handle of a result without photon records)
                self._call("clsimhip_release_result", ptr)
            result = ConversionResult((ident.value, np.zeros(0, dtype=PHOTON_DTYPE), (lambda: None)))
        else:
            buf = (C.c_char * (n.value * 80)).from_address(ptr.value)
            view = np.frombuffer(buf, dtype=PHOTON_DTYPE)
            view.flags.writeable = False
            result = ConversionResult((ident.value, view, (lambda: self._call("clsimhip_release_result", ptr))))
        self._attach_mcpes(result, mcpes)
        self._attach_pmt_hits(result, pmt_hits)
        self._attach_frame_photons(result, fp)
        self._attach_cable_shadow(result, shadow)
        self._attach_event_statistics(result, es)
        return result

    def _attach_pmt_hits(self, result, pmt_hits):
        if self._pmt_series and pmt_hits is not None:
            result.pmt_hits, result.pmt_series, result.masked = pmt_hits
        else:
            result.pmt_hits = pmt_hits

    def _attach_mcpes(self, result, mcpes):
        if self._series and mcpes is not None:
            result.mcpes, result.series, result.masked = mcpes[:3]
            if self._merging:
                result.merged, result.merged_series, result.parents, result.parent_ranges = mcpes[3]
        else:
            result.mcpes = mcpes

    def _size(self, name):
        v = C.c_size_t()
        self._call(name, C.byref(v))
        return v.value

    def GetWorkgroupSize(self): return self._size("clsimhip_get_workgroup_size")
    def GetMaxNumWorkitems(self): return self._size("clsimhip_get_max_num_workitems")
    def QueueSize(self): return self._size("clsimhip_queue_size")

    def MorePhotonsAvailable(self):
        v = C.c_int()
        self._call("clsimhip_more_photons_available", C.byref(v))
        return bool(v.value)

    def GetStatistics(self):
        out = (C.c_double * 8)()
        self._call("clsimhip_get_statistics", out)
        keys = ["TotalDeviceTime", "TotalHostTime", "NumKernelCalls", "TotalNumPhotonsGenerated",
                "TotalNumPhotonsAtDOMs", "AverageDeviceTimePerPhoton", "AverageHostTimePerPhoton", "DeviceUtilization"]
        return dict(zip(keys, list(out)))

    # the accessors of the concrete class (OpenCL.h:138-258, :377-381; times in nanoseconds)
    def GetTotalDeviceTime(self): return self.GetStatistics()["TotalDeviceTime"]
    def GetTotalHostTime(self): return self.GetStatistics()["TotalHostTime"]
    def GetNumKernelCalls(self): return int(self.GetStatistics()["NumKernelCalls"])
    def GetTotalNumPhotonsGenerated(self): return int(self.GetStatistics()["TotalNumPhotonsGenerated"])
    def GetTotalNumPhotonsAtDOMs(self): return int(self.GetStatistics()["TotalNumPhotonsAtDOMs"])

    # ---- tuning (include/clsimhip.h: clsimhip_set_tuning; no result depends on it) ----
    _KERNELS = {"auto": 0, "pool": 1, "classic": 2}

    def SetTuning(self, key, value):
        """clsimhip_set_tuning(key, value); "kernel" also takes "auto" | "pool" | "classic"."""
        if key == "kernel" and isinstance(value, str):
            value = self._KERNELS[value]
        self._call("clsimhip_set_tuning", key.encode(), int(value))

    def GetTuning(self, key):
        v = C.c_longlong()
        self._call("clsimhip_get_tuning", key.encode(), C.byref(v))
        return v.value

    def _option(self, which):
        v = C.c_double()
        self._call("clsimhip_get_option", int(which), C.byref(v))
        return v.value

    def GetEnableDoubleBuffering(self): return self._option(0) != 0.0
    def GetDoublePrecision(self): return self._option(1) != 0.0
    def GetStopDetectedPhotons(self): return self._option(2) != 0.0
    def GetSaveAllPhotons(self): return self._option(3) != 0.0
    def GetSaveAllPhotonsPrescale(self): return self._option(4)
    def GetFixedNumberOfAbsorptionLengths(self): return self._option(5)
    def GetDOMPancakeFactor(self): return self._option(6)
    def GetPhotonHistoryEntries(self): return int(self._option(7))

    # ---- device-resident path / introspection ----
    def PropagateDevice(self, d_steps, n, d_photons, capacity, d_hit_count, stream=0, rng_offset=0):
        self._call("clsimhip_propagate_device", C.c_void_p(d_steps), int(n), int(rng_offset), C.c_void_p(d_photons),
                   int(capacity), C.c_void_p(d_hit_count), C.c_void_p(stream))

    def SetConcurrentDeviceLaunches(self, k):
        """k device-path launches in flight on k streams (disjoint rng_offset ranges): each sizes its grid for 1/k of the chip"""
        self._call("clsimhip_set_concurrent_device_launches", int(k))

    def ReplaceIndicesWithIDs(self, photons):
        photons = np.ascontiguousarray(photons, dtype=PHOTON_DTYPE)
        self._call("clsimhip_replace_indices_with_ids", photons.ctypes.data_as(C.c_void_p), len(photons))
        return photons

    def KernelTimeMs(self, reset=False):
        total, launches = C.c_double(), C.c_uint64()
        self._call("clsimhip_kernel_time_ms", int(bool(reset)), C.byref(total), C.byref(launches))
        return total.value, launches.value

    def GetTable(self, name):
        n = self._lib.clsimhip_get_table(self._h, name.encode(), None, 0)
        if n < 0:
            _check(int(n), self._h)
        out = np.zeros(n, dtype=np.float64)
        self._lib.clsimhip_get_table(self._h, name.encode(), _dp(out), n)
        return out

    def KernelForBunch(self, n_steps):
        """'pool' or 'classic': the scheduling the propagation kernel runs with for a bunch of n_steps steps"""
        v = C.c_int32()
        self._call("clsimhip_kernel_for_bunch", int(n_steps), C.byref(v))
        return "pool" if v.value else "classic"

    def UsesPooledKernel(self):
        v = C.c_int32()
        self._call("clsimhip_uses_pooled_kernel", C.byref(v))
        return bool(v.value)

    def GetLastLaunch(self):
        """clsimhip_get_last_launch: the kernel instantiation the last launch dispatched to, as a dict
        {family: 'classic' | 'keep' | 'pool' | 'pool_keep', lengths: 'constant' | 'icecube' | 'table', tilt, aniso, flasher, fast};
        None before the first launch"""
        out = (C.c_int * 6)()
        self._call("clsimhip_get_last_launch", out)
        return _lib.launched_dict(out)

    BAKED_STATES = {0: "unused", 1: "baked", 2: "fallback"}

    def GetBakedInfo(self):
        """clsimhip_baked_info: {state: 'unused' | 'baked' | 'fallback', key, why} of the last launch that asked for the pooled kernel
        compiled for this configuration (tuning "baked_kernel")"""
        state, key, why = C.c_int(), C.create_string_buffer(33), C.create_string_buffer(4096)
        self._call("clsimhip_baked_info", C.byref(state), key, why, len(why))
        return {"state": self.BAKED_STATES[state.value], "key": key.value.decode(), "why": why.value.decode(errors="replace")}

    def CompileBakedKernel(self, arch="gfx950", flags=None, code_path=None):
        """clsimhip_baked_compile (after Compile(), no GPU needed): {compiled, key, seconds, why}; the code object goes to code_path"""
        key, why, seconds = C.create_string_buffer(33), C.create_string_buffer(4096), C.c_double()
        r = self._lib.clsimhip_baked_compile(self._h, arch.encode(), None if flags is None else flags.encode(),
                                             None if code_path is None else os.fsencode(code_path), key, C.byref(seconds), why, len(why))
        if r < 0:
            _check(int(r), self._h)
        return {"compiled": bool(r), "key": key.value.decode(), "seconds": seconds.value, "why": why.value.decode(errors="replace")}

    # ---- the reference's tester classes (private/test/I3CLSim*Tester): single functions evaluated on the device ----
    EVAL = {"lengths": 0, "refraction": 1, "wavelength_bias": 2, "tilt": 3, "abs_len_scaling": 4, "pre_scatter_transform": 5,
            "post_scatter_transform": 6}
    EVAL_RANDOM = {"uniform": 0, "wavelength": 1, "scattering_cosine": 2}

    def EvaluateOnDevice(self, what, values, layer=0, fast=False):
        """what: 'lengths' (values = wavelengths -> columns absorption, scattering length of `layer`), 'refraction' (-> phase
        index, group velocity), 'wavelength_bias', 'tilt' (values = positions (n, 3)), 'abs_len_scaling', 'pre_scatter_transform',
        'post_scatter_transform' (values = directions (n, 3) -> (n, 3)).  Returns float32 (n, 4)."""
        v = np.asarray(values, dtype=np.float32)
        inp = np.zeros((len(v), 4), dtype=np.float32)
        if v.ndim == 1:
            inp[:, 0] = v
        else:
            inp[:, :v.shape[1]] = v
        out = np.zeros_like(inp)
        self._call("clsimhip_eval_device_function", self.EVAL[what], int(layer), int(bool(fast)), inp.ctypes.data_as(C.c_void_p), len(inp),
                   out.ctypes.data_as(C.c_void_p))
        return out

    def SampleOnDevice(self, what, x, a, draws, generator=0, fast=False):
        """what: 'uniform', 'wavelength' (of `generator`), 'scattering_cosine'; one work item per stream (x[i], a[i]), `draws`
        values each.  Returns (values (n_streams, draws), final stream states)."""
        xs = np.ascontiguousarray(x, dtype=np.uint64).copy()
        a32 = np.ascontiguousarray(a, dtype=np.uint32)
        out = np.zeros((len(xs), int(draws)), dtype=np.float32)
        self._call("clsimhip_eval_device_random", self.EVAL_RANDOM[what], int(generator), int(bool(fast)), xs.ctypes.data_as(C.c_void_p),
                   a32.ctypes.data_as(C.c_void_p), len(xs), int(draws), out.ctypes.data_as(C.c_void_p))
        return out, xs

    def GetRNGState(self, count):
        x = np.zeros(count, dtype=np.uint64)
        self._call("clsimhip_get_rng_state", x.ctypes.data_as(C.c_void_p), count)
        return x


def initializeHIP(device, geometry, medium, wavelengthGenerationBias, wavelengthGenerators,
                  enableDoubleBuffering=False, doublePrecision=False, stopDetectedPhotons=True, saveAllPhotons=False,
                  saveAllPhotonsPrescale=0.01, fixedNumberOfAbsorptionLengths=float("nan"), pancakeFactor=1.0,
                  photonHistoryEntries=0, limitWorkgroupSize=0, approximateNumberOfWorkItems=262144,
                  seed=12345, streams=None, tuning=None, mcpeGenerator=None, keepPhotons=True, mcpeSeries=False, pmtHitGenerator=None, mcpeMergeWindow=None, pmtSeries=False,
                  framePhotons=False, cableShadow=None, eventStatistics=False):
    """Canonical configuration sequence, I3CLSimModuleHelper::initializeOpenCL
    (ModuleHelper.cxx:303-372).  tuning: {key: value} for clsimhip_set_tuning, applied before Compile().
    mcpeGenerator: an MCPEGenerator that turns every bunch's photons into MCPEs on the GPU (result attribute `mcpes`);
    keepPhotons=False then leaves the photon records on the device; mcpeSeries=True sorts them into per-frame, per-DOM series;
    mcpeMergeWindow=w then merges the records of a series within w of their group's opener (SetMCPEMerging).
    pmtHitGenerator: a PMTHitGenerator instead, for modules with several PMTs (result attribute `pmt_hits`; keepPhotons as above);
    pmtSeries=True sorts its hits into per-frame, per-module, per-PMT series (SetPMTSeries).
    framePhotons=True files the detected photons themselves into per-frame, per-module sorted series (SetFramePhotons; keepPhotons as
    above).  cableShadow: a CableShadow whose cylinders shadow detected photons before any of those stages (SetCableShadow).
    eventStatistics=True counts photons generated and at DOMs per particle, with exact weight sums (SetEventStatistics)."""
    conv = I3CLSimStepToPhotonConverterHIP(device)
    for key, value in (tuning or {}).items():
        conv.SetTuning(key, value)
    conv.SetWlenGenerators(wavelengthGenerators)
    conv.SetWlenBias(wavelengthGenerationBias)
    conv.SetMediumProperties(medium)
    conv.SetGeometry(geometry)
    conv.SetEnableDoubleBuffering(enableDoubleBuffering)
    conv.SetDoublePrecision(doublePrecision)
    conv.SetStopDetectedPhotons(stopDetectedPhotons)
    conv.SetSaveAllPhotons(saveAllPhotons)
    conv.SetSaveAllPhotonsPrescale(saveAllPhotonsPrescale)
    conv.SetFixedNumberOfAbsorptionLengths(fixedNumberOfAbsorptionLengths)
    conv.SetDOMPancakeFactor(pancakeFactor)
    conv.SetPhotonHistoryEntries(photonHistoryEntries)
    if mcpeGenerator is not None:
        conv.SetMCPEGenerator(mcpeGenerator, keepPhotons)
    if mcpeSeries:
        conv.SetMCPESeries(True)
    if mcpeMergeWindow is not None:
        conv.SetMCPEMerging(mcpeMergeWindow)
    if pmtHitGenerator is not None:
        conv.SetPMTHitGenerator(pmtHitGenerator, keepPhotons)
    if pmtSeries:
        conv.SetPMTSeries(True)
    if framePhotons:
        conv.SetFramePhotons(True, keepPhotons)
    if cableShadow is not None:
        conv.SetCableShadow(cableShadow)
    if eventStatistics:
        conv.SetEventStatistics(True)
    conv.Compile()
    max_wg = conv.GetMaxWorkgroupSize()
    if limitWorkgroupSize:
        max_wg = min(limitWorkgroupSize, max_wg)
    conv.SetWorkgroupSize(max_wg)
    wg = max_wg
    max_items = (int(approximateNumberOfWorkItems) // wg) * wg
    if max_items == 0:
        max_items = wg
    conv.SetMaxNumWorkitems(max_items)
    if streams is not None:
        conv.InitializeWithStreams(streams[0][:max_items], streams[1][:max_items])
    else:
        conv.Initialize(seed)
    return conv


# ---- step producer on the GPU (clsimhip_generate_steps*, csrc/steps_kernel.hip) ----
REQUEST_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("time", "<f4"), ("dx", "<f4"), ("dy", "<f4"), ("dz", "<f4"),
                          ("length", "<f4"), ("pa", "<f4"), ("pb", "<f4"), ("kind", "<u4"), ("identifier", "<u4"),
                          ("photons_per_step", "<u4"), ("num_photons_in_last_step", "<u4"), ("num_steps", "<u8")])
STEPS_CASCADE, STEPS_MUON_CASCADE, STEPS_MUON = 0, 1, 2


def CountGeneratedSteps(requests, granularity=1):
    req = np.ascontiguousarray(requests, dtype=REQUEST_DTYPE)
    steps, padded = C.c_size_t(), C.c_size_t()
    _check(_lib.load().clsimhip_count_generated_steps(req.ctypes.data_as(C.POINTER(_lib.StepRequest)), len(req), int(granularity),
                                                      C.byref(steps), C.byref(padded)))
    return steps.value, padded.value


def GenerateSteps(requests, seed, granularity=1, device=0):
    """Steps of a list of step requests (the reference's CascadeStepData_t / MuonStepData_t queue entries,
    I3CLSimLightSourceToStepConverterPPC.cxx:524-551, 785-842), generated on the GPU, as a host array."""
    req = np.ascontiguousarray(requests, dtype=REQUEST_DTYPE)
    _, padded = CountGeneratedSteps(req, granularity)
    out = np.zeros(padded, dtype=STEP_DTYPE)
    got = C.c_size_t()
    _check(_lib.load().clsimhip_generate_steps(int(device), req.ctypes.data_as(C.POINTER(_lib.StepRequest)), len(req), int(seed),
                                               int(granularity), out.ctypes.data_as(C.c_void_p), len(out), C.byref(got)))
    return out


def GenerateStepsDevice(requests, seed, d_steps, capacity, granularity=1, device=0, stream=0):
    """The same into device memory (address d_steps, room for `capacity` steps); returns the padded step count."""
    req = np.ascontiguousarray(requests, dtype=REQUEST_DTYPE)
    got = C.c_size_t()
    _check(_lib.load().clsimhip_generate_steps_device(int(device), req.ctypes.data_as(C.POINTER(_lib.StepRequest)), len(req), int(seed),
                                                      int(granularity), C.c_void_p(d_steps), int(capacity), C.c_void_p(stream), C.byref(got)))
    return got.value


# ---- particle -> step requests (I3CLSimLightSourceToStepConverterPPC front end, csrc/lightsource.cpp) ----
PARTICLE_DTYPE = np.dtype([("type", "<i4"), ("shape", "<i4"), ("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("time", "<f8"),
                           ("dx", "<f8"), ("dy", "<f8"), ("dz", "<f8"), ("energy", "<f8"), ("length", "<f8"),
                           ("identifier", "<u4"), ("reserved", "<u4")])
assert PARTICLE_DTYPE.itemsize == 88


class ParticleType:
    """I3Particle::ParticleType values (dataclasses): PDG codes and IceCube's codes for stochastic losses"""
    Gamma, EMinus, EPlus, MuMinus, MuPlus, TauMinus, TauPlus = 22, 11, -11, 13, -13, 15, -15
    Pi0, PiPlus, PiMinus, K0_Long, KPlus, KMinus, K0_Short = 111, 211, -211, 130, 321, -321, 310
    PPlus, PMinus, Neutron = 2212, -2212, 2112
    Brems, DeltaE, PairProd, NuclInt, Hadrons = -2000001001, -2000001002, -2000001003, -2000001004, -2000001006


SHAPE_OTHER, SHAPE_CASCADE_SEGMENT = 0, 1


class I3CLSimLightSourceToStepConverterPPC:
    """Front end of the reference's converter (private/clsim/I3CLSimLightSourceToStepConverterPPC.cxx:51-132, 188-470): particles in,
    step requests out; GenerateSteps / GenerateStepsDevice make the steps on the GPU."""

    def __init__(self, photonsPerStep=200, highPhotonsPerStep=2000, useHighPhotonsPerStepStartingFromNumPhotons=1.0e9):
        if photonsPerStep <= 0 or highPhotonsPerStep <= 0:
            raise I3CLSimStepToPhotonConverter_exception("photonsPerStep may not be <= 0!")
        self._cfg = _lib.PPCConfig(int(photonsPerStep), int(highPhotonsPerStep), float(useHighPhotonsPerStepStartingFromNumPhotons), 1, 0, 0.9216, 0)
        self._bias = self._medium = self._h = None
        self._lib = _lib.load()

    def SetUseCascadeExtension(self, v):
        """may be called after Initialize(), as resources/tests/testCascadeExtension.py does (the library object is rebuilt)"""
        self._cfg.use_cascade_extension = int(bool(v))
        if self._h is not None:
            self._lib.clsimhip_ppc_destroy(self._h)
            self._h = None
            self.Initialize()

    def SetWlenBias(self, wlenBias):
        self._bias = wlenBias

    def SetMediumProperties(self, mediumProperties, density=0.9216):
        self._medium = mediumProperties
        self._cfg.medium_density = float(density)

    def SetRandomSeed(self, seed):
        self._cfg.seed = int(seed)

    def Initialize(self):
        if self._bias is None:
            raise I3CLSimStepToPhotonConverter_exception("WlenBias not set!")
        if self._medium is None:
            raise I3CLSimStepToPhotonConverter_exception("MediumProperties not set!")
        h = C.c_void_p()
        d = self._bias._desc()
        _check(self._lib.clsimhip_ppc_create(self._medium._h, C.byref(d), C.byref(self._cfg), C.byref(h)))
        self._h = h

    def __del__(self):
        try:
            if self._h:
                self._lib.clsimhip_ppc_destroy(self._h)
        except Exception:
            pass

    def IsInitialized(self):
        return self._h is not None

    def MeanPhotonsPerMeter(self, layer=0):
        v = C.c_double()
        _check(self._lib.clsimhip_ppc_photons_per_meter(self._h, int(layer), C.byref(v)))
        return v.value

    def EnqueueLightSources(self, particles):
        """particles: array of PARTICLE_DTYPE -> array of REQUEST_DTYPE (one per cascade, two per muon / tau)"""
        if self._h is None:
            raise I3CLSimStepToPhotonConverter_exception("I3CLSimLightSourceToStepConverterPPC is not initialized!")
        p = np.ascontiguousarray(particles, dtype=PARTICLE_DTYPE)
        out = np.zeros(2 * len(p), dtype=REQUEST_DTYPE)
        n = C.c_size_t()
        _check(self._lib.clsimhip_ppc_enqueue(self._h, p.ctypes.data_as(C.c_void_p), len(p), out.ctypes.data_as(C.POINTER(_lib.StepRequest)),
                                              len(out), C.byref(n)))
        return out[:n.value]


def ShowerParameters(particleType, energy, density=0.9216):
    """(a, b [m], emScale, emScaleSigma) of I3SimConstants::ShowerParameters as restated in csrc/lightsource.cpp"""
    out = (C.c_double * 4)()
    _check(_lib.load().clsimhip_shower_parameters(int(particleType), float(energy), float(density), out))
    return tuple(out)


# ---- flasher step producer (I3CLSimLightSourceToStepConverterFlasher) ----
FLASHER_REQUEST_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("time", "<f4"), ("dx", "<f4"), ("dy", "<f4"), ("dz", "<f4"),
                                  ("sigma_polar", "<f4"), ("sigma_azimuthal", "<f4"), ("pulse_width", "<f4"), ("identifier", "<u4"),
                                  ("source_type", "<u4"), ("num_photons_with_bias", "<u8")])
assert FLASHER_REQUEST_DTYPE.itemsize == 56
DIST_CONSTANT, DIST_NORMAL, DIST_UNIFORM, DIST_FLASHER_TIME_PROFILE = 0, 1, 2, 3


FLASHER_PULSE_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("time", "<f4"), ("dx", "<f4"), ("dy", "<f4"), ("dz", "<f4"),
                                ("sigma_polar", "<f4"), ("sigma_azimuthal", "<f4"), ("pulse_width", "<f4"), ("identifier", "<u4"),
                                ("source_type", "<u4"), ("num_photons_no_bias", "<f8")])
assert FLASHER_PULSE_DTYPE.itemsize == 56


def FlasherPhotonNumberCorrectionFactor(wlenBias, spectrumNoBias=None, peakWavelength=None, fromWlen=265e-9, toWlen=675e-9):
    """PhotonNumberCorrectionFactorAfterBias (ConverterUtils.cxx:113-214): spectrumNoBias = I3CLSimFunctionFromTable, or None with
    peakWavelength for an I3CLSimFunctionDeltaPeak"""
    v = C.c_double()
    b = wlenBias._desc()
    if spectrumNoBias is None:
        _check(_lib.load().clsimhip_flasher_correction_factor(None, float(peakWavelength), C.byref(b), float(fromWlen), float(toWlen), C.byref(v)))
    else:
        sp = spectrumNoBias._desc()
        _check(_lib.load().clsimhip_flasher_correction_factor(C.byref(sp), 0.0, C.byref(b), float(fromWlen), float(toWlen), C.byref(v)))
    return v.value


def EnqueueFlasherPulses(pulses, correctionFactor, seed=0):
    """I3CLSimLightSourceToStepConverterFlasher::EnqueueLightSource (Flasher.cxx:214-265) for an array of FLASHER_PULSE_DTYPE:
    the converter's queue entries (FLASHER_REQUEST_DTYPE) with the photon numbers after bias drawn"""
    p = np.ascontiguousarray(pulses, dtype=FLASHER_PULSE_DTYPE)
    out = np.zeros(len(p), dtype=FLASHER_REQUEST_DTYPE)
    n = C.c_size_t()
    _check(_lib.load().clsimhip_flasher_enqueue(float(correctionFactor), int(seed), p.ctypes.data_as(C.c_void_p), len(p),
                                                out.ctypes.data_as(C.c_void_p), len(out), C.byref(n)))
    return out[:n.value]


def FlasherStepConverterConfig(angularProfileDistributionPolar, angularProfileDistributionAzimuthal, timeDelayDistribution,
                               interpretAngularDistributionsInPolarCoordinates=False, photonsPerStep=400, maxBunchSize=512000,
                               bunchSizeGranularity=512):
    """Constructor arguments of I3CLSimLightSourceToStepConverterFlasher (Flasher.h; defaults Flasher.cxx:46-48); a
    distribution is (kind, value): (DIST_NORMAL, mean), (DIST_CONSTANT, 0), (DIST_UNIFORM, from), (DIST_FLASHER_TIME_PROFILE, 0).
    python/GetFlasherParameterizationList.py: LEDs = normal(0) / normal(0) / time profile, not polar; standard candles =
    constant / uniform(0) / normal(2 ns), polar."""
    c = _lib.FlasherConfig()
    for name, d in (("polar", angularProfileDistributionPolar), ("azimuthal", angularProfileDistributionAzimuthal), ("time_delay", timeDelayDistribution)):
        f = getattr(c, name)
        f.kind, f.value = int(d[0]), float(d[1])
    c.interpret_in_polar_coordinates = 1 if interpretAngularDistributionsInPolarCoordinates else 0
    c.photons_per_step, c.max_bunch_size, c.bunch_size_granularity = int(photonsPerStep), int(maxBunchSize), int(bunchSizeGranularity)
    return c


def CountFlasherSteps(config, requests):
    req = np.ascontiguousarray(requests, dtype=FLASHER_REQUEST_DTYPE)
    total, real = C.c_size_t(), C.c_size_t()
    _check(_lib.load().clsimhip_count_flasher_steps(C.byref(config), req.ctypes.data_as(C.c_void_p), len(req), C.byref(total), C.byref(real)))
    return total.value, real.value


def GenerateFlasherSteps(config, requests, seed, device=0):
    """All steps of the given flasher pulses (MakeSteps called until every pulse is used up), made on the GPU."""
    req = np.ascontiguousarray(requests, dtype=FLASHER_REQUEST_DTYPE)
    total, _ = CountFlasherSteps(config, req)
    out = np.zeros(total, dtype=STEP_DTYPE)
    n = C.c_size_t()
    _check(_lib.load().clsimhip_generate_flasher_steps(int(device), C.byref(config), req.ctypes.data_as(C.c_void_p), len(req), int(seed),
                                                       out.ctypes.data_as(C.c_void_p), total, C.byref(n)))
    return out[:n.value]


def GenerateFlasherStepsDevice(config, requests, seed, d_steps, capacity, device=0, stream=0):
    req = np.ascontiguousarray(requests, dtype=FLASHER_REQUEST_DTYPE)
    n = C.c_size_t()
    _check(_lib.load().clsimhip_generate_flasher_steps_device(int(device), C.byref(config), req.ctypes.data_as(C.c_void_p), len(req), int(seed),
                                                              C.c_void_p(int(d_steps)), int(capacity), C.c_void_p(int(stream)), C.byref(n)))
    return n.value


def FlasherTimeProfile(pulseWidthNs):
    """(density, cumulative) tables of the time delay distribution of one pulse width (240 points at 0.5 ns)."""
    d, c = np.zeros(240, dtype=np.float32), np.zeros(240, dtype=np.float32)
    _check(_lib.load().clsimhip_flasher_time_profile(float(pulseWidthNs), d.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p)))
    return d, c


# ---- muon slicer and series relabel (include/clsimhip.h: I3MuonSlicer and I3MuonSliceRemoverAndPulseRelabeler) ----
TREE_PARTICLE_DTYPE = np.dtype([("particle", PARTICLE_DTYPE), ("speed", "<f8"), ("parent", "<i4"), ("flags", "<u4")])
MMC_TRACK_DTYPE = np.dtype([("identifier", "<u4"), ("reserved", "<u4"), ("Ei", "<f8"), ("Ef", "<f8"), ("ti", "<f8"), ("tf", "<f8")])
RELABEL_DTYPE = np.dtype([("from", "<u4"), ("to", "<u4")])
assert TREE_PARTICLE_DTYPE.itemsize == 104 and MMC_TRACK_DTYPE.itemsize == 40 and RELABEL_DTYPE.itemsize == 8
TREE_DARK = 1
SLICER_COUNTERS = ("off_track", "energy_reset", "stops_before_start", "zero_duration", "long_slice")
RELABEL_COUNTERS = ("relabelled", "tie_overflow")
RELABEL_COUNTS = ("records", "series", "relabelled", "reserved", "tie_overflow")


def slice_muons(tree, tracks, first_slice_identifier):
    """(tree, relabel, counters): I3MuonSlicer on a flattened tree.  tree: TREE_PARTICLE_DTYPE in depth-first pre-order; tracks:
    MMC_TRACK_DTYPE; the k-th slice of the output takes identifier first_slice_identifier + k.  relabel: RELABEL_DTYPE, (slice ->
    muon), ascending in `from`; counters = {name: count} (SLICER_COUNTERS).  EnqueueLightSources takes the output's `particle` field
    of the nodes without TREE_DARK."""
    tree = np.ascontiguousarray(tree, dtype=TREE_PARTICLE_DTYPE)
    tracks = np.ascontiguousarray(tracks, dtype=MMC_TRACK_DTYPE)
    lib = _lib.load()
    n_out, n_relabel, counters = C.c_size_t(), C.c_size_t(), np.zeros(5, dtype=np.uint64)
    out, relabel = np.zeros(0, dtype=TREE_PARTICLE_DTYPE), np.zeros(0, dtype=RELABEL_DTYPE)
    for _ in range(2):                  # sizes first, as with clsimhip_ppc_enqueue
        _check(lib.clsimhip_slice_muons(tree.ctypes.data_as(C.c_void_p), len(tree), tracks.ctypes.data_as(C.c_void_p), len(tracks), int(first_slice_identifier),
                                        out.ctypes.data_as(C.c_void_p), len(out), C.byref(n_out), relabel.ctypes.data_as(C.c_void_p), len(relabel),
                                        C.byref(n_relabel), counters.ctypes.data_as(C.c_void_p)))
        if n_out.value <= len(out) and n_relabel.value <= len(relabel):
            break
        out, relabel = np.zeros(n_out.value, dtype=TREE_PARTICLE_DTYPE), np.zeros(n_relabel.value, dtype=RELABEL_DTYPE)
    return out[:n_out.value], relabel[:n_relabel.value], dict(zip(SLICER_COUNTERS, (int(c) for c in counters)))


class SeriesRelabeler:
    """RELABEL(X, map) of include/clsimhip.h for the two series forms and the merging stage's parent table.  map: RELABEL_DTYPE (or
    pairs), strictly ascending in `from`, no `to` among the `from`s -- slice_muons' relabel table."""

    def __init__(self, map):
        self.map = np.ascontiguousarray(map, dtype=RELABEL_DTYPE).reshape(-1)
        self._lib = _lib.load()

    def _host(self, fn, records, series, dtype):
        records = np.ascontiguousarray(records, dtype=dtype)
        series = np.ascontiguousarray(series, dtype=MCPE_SERIES_DTYPE)
        out, counters, kept = np.zeros(len(records), dtype=dtype), np.zeros(2, dtype=np.uint64), C.c_size_t()
        _check(fn(records.ctypes.data_as(C.c_void_p), len(records), series.ctypes.data_as(C.c_void_p), len(series), self.map.ctypes.data_as(C.c_void_p),
                  len(self.map), out.ctypes.data_as(C.c_void_p), counters.ctypes.data_as(C.c_void_p), C.byref(kept)))
        counters = dict(zip(RELABEL_COUNTERS, (int(c) for c in counters)))
        return (out, series.copy(), counters) if not counters["tie_overflow"] else (out[:0], series[:0].copy(), counters)

    def mcpe_series_host(self, records, series):
        """(records, series, counters): the host twin on MCPE_DTYPE records; nothing is delivered after a TIE_OVERFLOW"""
        return self._host(self._lib.clsimhip_mcpe_series_relabel_host, records, series, MCPE_DTYPE)

    def frame_photons_host(self, records, series):
        """(records, series, counters): the host twin on FRAME_PHOTON_DTYPE records"""
        return self._host(self._lib.clsimhip_frame_photons_relabel_host, records, series, FRAME_PHOTON_DTYPE)

    def workspace_bytes(self, capacity, record_bytes):
        return int(self._lib.clsimhip_series_relabel_workspace_bytes(int(capacity), len(self.map), int(record_bytes)))

    def _device(self, fn, d_records, d_series, d_counts, capacity, d_out_records, d_out_series, d_out_counts, d_workspace, workspace_bytes, device, stream):
        _check(fn(int(device), C.c_void_p(d_records), C.c_void_p(d_series), C.c_void_p(d_counts), int(capacity), self.map.ctypes.data_as(C.c_void_p), len(self.map),
                  C.c_void_p(d_out_records), C.c_void_p(d_out_series), C.c_void_p(d_out_counts), C.c_void_p(d_workspace), int(workspace_bytes), C.c_void_p(stream)))

    def mcpe_series_device(self, d_records, d_series, d_counts, capacity, d_out_records, d_out_series, d_out_counts, d_workspace, workspace_bytes,
                           device=0, stream=0):
        """the kernels on a device-resident series form (addresses; pairs with MakeSeriesDevice, a union or a store's DrainDevice);
        d_out_counts: five uint32 (RELABEL_COUNTS); d_workspace: workspace_bytes(capacity, 16) bytes; asynchronous on `stream`"""
        self._device(self._lib.clsimhip_mcpe_series_relabel_device, d_records, d_series, d_counts, capacity, d_out_records, d_out_series, d_out_counts,
                     d_workspace, workspace_bytes, device, stream)

    def frame_photons_device(self, d_records, d_series, d_counts, capacity, d_out_records, d_out_series, d_out_counts, d_workspace, workspace_bytes,
                             device=0, stream=0):
        """the same on frame photons (48-byte records; workspace_bytes(capacity, 48))"""
        self._device(self._lib.clsimhip_frame_photons_relabel_device, d_records, d_series, d_counts, capacity, d_out_records, d_out_series, d_out_counts,
                     d_workspace, workspace_bytes, device, stream)

    def parents_host(self, parents, ranges):
        """(parents, ranges): the merging stage's parent table under the map -- relabelled, sorted by (id, index) per series, duplicates
        dropped.  On the device the table comes from merging BEHIND the relabel stage instead."""
        parents = np.ascontiguousarray(parents, dtype=MCPE_PARENT_DTYPE)
        ranges = np.ascontiguousarray(ranges, dtype=MCPE_PARENT_RANGE_DTYPE)
        out, out_ranges, n = np.zeros(len(parents), dtype=MCPE_PARENT_DTYPE), np.zeros(len(ranges), dtype=MCPE_PARENT_RANGE_DTYPE), C.c_size_t()
        _check(self._lib.clsimhip_mcpe_parents_relabel_host(parents.ctypes.data_as(C.c_void_p), ranges.ctypes.data_as(C.c_void_p), len(ranges),
                                                            self.map.ctypes.data_as(C.c_void_p), len(self.map), out.ctypes.data_as(C.c_void_p),
                                                            out_ranges.ctypes.data_as(C.c_void_p), C.byref(n)))
        return out[:n.value], out_ranges


EVENT_STATISTICS_STORE_COUNTERS = ("relabelled", "empty_dropped")
# the five output counts of the event statistics store's device stages (include/clsimhip.h: "Event statistics frame store")
EVENT_STATISTICS_CANONICAL_COUNTS = ("records", "series", "relabelled", "empty_dropped", "overflow")
EVENT_STATISTICS_COMBINE_COUNTS = ("records", "series", "malformed_a", "malformed_b", "overflow")


def _statistics(records):
    return np.ascontiguousarray(records, dtype=EVENT_STATISTICS_DTYPE).reshape(-1)


def _relabel_map(map):
    return np.zeros(0, dtype=RELABEL_DTYPE) if map is None else np.ascontiguousarray(map, dtype=RELABEL_DTYPE).reshape(-1)


def _address(array):
    return C.c_void_p(array.ctypes.data if len(array) else None)


class EventStatisticsStore:
    """The event statistics records of several bunches accumulate per frame and particle as exact sums; finished frames leave
    (clsimhip_event_statistics_store; include/clsimhip.h: "Event statistics frame store"): what MCPEFrameStore is for MCPEs, for
    EVENT_STATISTICS_DTYPE records, with a relabel map (RELABEL_DTYPE, slice_muons' table) that folds slices into their muon when a
    bunch is added or when a frame is drained.  device=None: a host store, which needs no GPU; device=k: the state lives in HBM of
    GPU k.  Call Add (or AddDevice) per result and Drain with the last frame no bunch in flight can still touch."""

    def __init__(self, capacity, device=None):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.capacity, self.device = int(capacity), device
        _check(self._lib.clsimhip_event_statistics_store_create(-1 if device is None else int(device), self.capacity, C.byref(self._h)))

    def __del__(self):
        try:
            if self._h:
                self._lib.clsimhip_event_statistics_store_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def Add(self, records, map=None):
        """one bunch in host memory: any list of records (a result's event statistics as they come, zeros included)"""
        records, map = _statistics(records), _relabel_map(map)
        _check(self._lib.clsimhip_event_statistics_store_add_host(self._h, _address(records), len(records), _address(map), len(map)))

    def AddDevice(self, d_records, d_count, capacity, map=None, stream=0):
        """one bunch in HBM (addresses: EventStatistics.MakeDevice's d_out, and word 3 of its d_counters as the count); asynchronous
        on `stream`"""
        map = _relabel_map(map)
        _check(self._lib.clsimhip_event_statistics_store_add_device(self._h, C.c_void_p(d_records), C.c_void_p(d_count), int(capacity), _address(map), len(map),
                                                                    C.c_void_p(stream)))

    def Size(self, last_frame=ALL_FRAMES):
        """records of the frames <= last_frame, before a drain's map folds them: what a Drain's output must hold; waits"""
        n = C.c_size_t()
        _check(self._lib.clsimhip_event_statistics_store_size(self._h, int(last_frame), C.byref(n)))
        return n.value

    def Drain(self, last_frame=ALL_FRAMES, map=None):
        """the records of the frames <= last_frame under the map, which leave the store; waits"""
        n, map = self.Size(last_frame), _relabel_map(map)
        records, got = np.zeros(n, dtype=EVENT_STATISTICS_DTYPE), C.c_size_t()
        _check(self._lib.clsimhip_event_statistics_store_drain_host(self._h, int(last_frame), _address(map), len(map), _address(records), n, C.byref(got)))
        return records[:got.value]

    def DrainDevice(self, last_frame, d_out, d_counts, capacity, map=None, stream=0):
        """the frames <= last_frame move to the caller's device buffer under the map (addresses; d_counts: five uint32,
        EVENT_STATISTICS_CANONICAL_COUNTS); asynchronous on `stream`"""
        map = _relabel_map(map)
        _check(self._lib.clsimhip_event_statistics_store_drain_device(self._h, int(last_frame), _address(map), len(map), C.c_void_p(d_out), C.c_void_p(d_counts),
                                                                      int(capacity), C.c_void_p(stream)))

    @staticmethod
    def CanonicalHost(records, map=None, capacity=None):
        """(records, counters): the host twin of CANON; counters = {name: count} (EVENT_STATISTICS_STORE_COUNTERS); capacity: of the
        output, len(records) by default"""
        records, map = _statistics(records), _relabel_map(map)
        capacity = len(records) if capacity is None else int(capacity)
        out, n, counters = np.zeros(capacity, dtype=EVENT_STATISTICS_DTYPE), C.c_size_t(), np.zeros(2, dtype=np.uint64)
        _check(_lib.load().clsimhip_event_statistics_canonical_host(_address(records), len(records), _address(map), len(map), _address(out), capacity, C.byref(n),
                                                                    counters.ctypes.data_as(C.c_void_p)))
        return out[:n.value], dict(zip(EVENT_STATISTICS_STORE_COUNTERS, (int(c) for c in counters)))

    @staticmethod
    def CombineHost(a, b, capacity=None):
        """the host twin of COMBINE of two statistics forms; capacity: of the output, len(a) + len(b) by default"""
        a, b = _statistics(a), _statistics(b)
        capacity = len(a) + len(b) if capacity is None else int(capacity)
        out, n = np.zeros(capacity, dtype=EVENT_STATISTICS_DTYPE), C.c_size_t()
        _check(_lib.load().clsimhip_event_statistics_combine_host(_address(a), len(a), _address(b), len(b), _address(out), capacity, C.byref(n)))
        return out[:n.value]

    @staticmethod
    def SplitHost(records, last_frame, head_capacity=None, tail_capacity=None):
        """(head, tail): the host twin of SPLIT -- the head holds the frames <= last_frame"""
        records = _statistics(records)
        head_capacity = len(records) if head_capacity is None else int(head_capacity)
        tail_capacity = len(records) if tail_capacity is None else int(tail_capacity)
        head, tail = np.zeros(head_capacity, dtype=EVENT_STATISTICS_DTYPE), np.zeros(tail_capacity, dtype=EVENT_STATISTICS_DTYPE)
        n_head, n_tail = C.c_size_t(), C.c_size_t()
        _check(_lib.load().clsimhip_event_statistics_split_host(_address(records), len(records), int(last_frame), _address(head), head_capacity, C.byref(n_head),
                                                                _address(tail), tail_capacity, C.byref(n_tail)))
        return head[:n_head.value], tail[:n_tail.value]

    @staticmethod
    def WorkspaceBytes(capacity_a, capacity_b):
        """bytes of d_workspace: CombineDevice of (capacity_a, capacity_b); CanonicalDevice of `capacity` records under a map of n_map
        entries takes (capacity, n_map)"""
        return int(_lib.load().clsimhip_event_statistics_store_workspace_bytes(int(capacity_a), int(capacity_b)))

    @staticmethod
    def CanonicalDevice(d_records, d_count, capacity, d_out, d_out_counts, out_capacity, d_workspace, workspace_bytes, map=None, device=0, stream=0):
        """the kernels on device-resident records (addresses; d_count: one uint32); d_out_counts: five uint32
        (EVENT_STATISTICS_CANONICAL_COUNTS); d_workspace: WorkspaceBytes(capacity, len(map)) bytes"""
        map = _relabel_map(map)
        _check(_lib.load().clsimhip_event_statistics_canonical_device(int(device), C.c_void_p(d_records), C.c_void_p(d_count), int(capacity), _address(map), len(map),
                                                                      C.c_void_p(d_out), C.c_void_p(d_out_counts), int(out_capacity), C.c_void_p(d_workspace),
                                                                      int(workspace_bytes), C.c_void_p(stream)))

    @staticmethod
    def CombineDevice(d_a, d_a_count, capacity_a, d_b, d_b_count, capacity_b, d_out, d_out_counts, out_capacity, d_workspace, workspace_bytes, device=0, stream=0):
        """the kernels on two device-resident statistics forms (addresses); d_out_counts: five uint32 (EVENT_STATISTICS_COMBINE_COUNTS);
        d_workspace: WorkspaceBytes(capacity_a, capacity_b) bytes"""
        _check(_lib.load().clsimhip_event_statistics_combine_device(int(device), C.c_void_p(d_a), C.c_void_p(d_a_count), int(capacity_a), C.c_void_p(d_b),
                                                                    C.c_void_p(d_b_count), int(capacity_b), C.c_void_p(d_out), C.c_void_p(d_out_counts),
                                                                    int(out_capacity), C.c_void_p(d_workspace), int(workspace_bytes), C.c_void_p(stream)))

    @staticmethod
    def SplitDevice(d_records, d_count, capacity, last_frame, d_head, d_head_counts, head_capacity, d_tail, d_tail_counts, tail_capacity, device=0, stream=0):
        """the split on a device-resident statistics form (addresses); d_head_counts / d_tail_counts: five uint32 each (records, 0, 0, 0,
        overflow)"""
        _check(_lib.load().clsimhip_event_statistics_split_device(int(device), C.c_void_p(d_records), C.c_void_p(d_count), int(capacity), int(last_frame),
                                                                  C.c_void_p(d_head), C.c_void_p(d_head_counts), int(head_capacity), C.c_void_p(d_tail),
                                                                  C.c_void_p(d_tail_counts), int(tail_capacity), C.c_void_p(stream)))
