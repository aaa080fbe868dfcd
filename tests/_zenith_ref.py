"""fp64 / numpy statement of the cosine of the solar zenith angle as csrc/zenith.hip defines it: the formulas of
makani/third_party/climt/zenith_angle_v2.py with the angles themselves (declination, right ascension, GMST mod 2 pi) and
every quantity in fp64.  Times are int64 UTC microseconds since the Unix epoch; lat / lon are 1-D, in degrees."""
import numpy as np

J2000_US = 946_728_000_000_000          # 2000-01-01T12:00:00 UTC
TIMES = ["1979-01-01T00:00", "2000-01-01T12:00", "2024-02-29T18:00", "2049-12-31T23:59:59.5"]


def times_us(stamps=TIMES):
    return np.array(stamps, dtype="datetime64[us]").astype(np.int64)


def time_scalars(t_us):
    """(declination, right ascension, gmst mod 2 pi) per time, radians"""
    jc = (np.asarray(t_us, dtype=np.int64) - J2000_US).astype(np.float64) / 86400.0e6 / 36525.0
    eps = np.deg2rad(23.0 + 26.0 / 60 + 21.406 / 3600.0
                     - (46.836769 * jc - 0.0001831 * jc**2 + 0.00200340 * jc**3 - 0.576e-6 * jc**4 - 4.34e-8 * jc**5) / 3600.0)
    anomaly = np.deg2rad(357.52910 + 35999.05030 * jc - 0.0001559 * jc * jc - 0.00000048 * jc * jc * jc)
    longitude = np.deg2rad(280.46645 + 36000.76983 * jc + 0.0003032 * jc * jc)
    eclon = longitude + np.deg2rad((1.914600 - 0.004817 * jc - 0.000014 * jc * jc) * np.sin(anomaly)
                                   + (0.019993 - 0.000101 * jc) * np.sin(2 * anomaly) + 0.000290 * np.sin(3 * anomaly))
    x, y, z = np.cos(eclon), np.cos(eps) * np.sin(eclon), np.sin(eps) * np.sin(eclon)
    r = np.sqrt(1.0 - z * z)
    theta = 67310.54841 + jc * (876600 * 3600 + 8640184.812866 + jc * (0.093104 - jc * 6.2e-5))
    return np.arctan2(z, r), 2.0 * np.arctan2(y, x + r), np.deg2rad(theta / 240.0) % (2 * np.pi)


def cos_zenith(t_us, lat_deg, lon_deg):
    """(*t_us.shape, H, W) fp64"""
    dec, ra, gmst = (v[..., None, None] for v in time_scalars(t_us))
    lat = np.deg2rad(np.asarray(lat_deg, dtype=np.float64))[:, None]
    lon = np.deg2rad(np.asarray(lon_deg, dtype=np.float64))[None, :]
    return np.sin(lat) * np.sin(dec) + np.cos(lat) * np.cos(dec) * np.cos(gmst - ra + lon)
