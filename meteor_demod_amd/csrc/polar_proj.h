/*
 * polar_proj.h — the polar stereographic projection of include/meteor_demod_amd_polar.h, once, for the host (csrc/polar_host.cpp) and
 * for the device (csrc/polar.hip): the same formulas in double on both.  Angles in radians here.  Free of the GPU runtime.
 */
#ifndef MDEMOD_POLAR_PROJ_H
#define MDEMOD_POLAR_PROJ_H

#include <math.h>

#ifdef __HIPCC__
#define POLAR_HD __host__ __device__ inline
#else
#define POLAR_HD inline
#endif

#define POLAR_A        6378137.0                       /* metres */
#define POLAR_F        (1.0 / 298.257223563)
#define POLAR_E2       (POLAR_F * (2.0 - POLAR_F))
#define POLAR_PI       3.14159265358979323846
#define POLAR_RAD      (POLAR_PI / 180.0)
#define POLAR_INV_TOL  1.0e-14
#define POLAR_INV_MAX  10

/* pole +1 or -1; lon0 in radians; scale = a m_c / t(phi_c): rho = scale t(phi) */
struct PolarProj {
	double lon0, scale;
	int pole;
};

/* t(phi) = tan(pi/4 - phi/2) / ((1 - e sin phi) / (1 + e sin phi))^(e/2) */
POLAR_HD double
polar_t(double phi)
{
	const double e = sqrt(POLAR_E2), es = e * sin(phi);
	return tan(POLAR_PI / 4.0 - phi / 2.0) / pow((1.0 - es) / (1.0 + es), e / 2.0);
}

/* lat_ts: the magnitude of the standard parallel, radians, 0 < lat_ts <= pi/2 (at pi/2 the scale is the limit 2 a / sqrt((1+e)^(1+e) (1-e)^(1-e))) */
POLAR_HD double
polar_scale(double lat_ts)
{
	const double e = sqrt(POLAR_E2);
	if (POLAR_PI / 2.0 - lat_ts < 1.0e-9) return 2.0 * POLAR_A / sqrt(pow(1.0 + e, 1.0 + e) * pow(1.0 - e, 1.0 - e));
	const double s = sin(lat_ts), m = cos(lat_ts) / sqrt(1.0 - POLAR_E2 * s * s);
	return POLAR_A * m / polar_t(lat_ts);
}

/* (phi, lam) to (E, N) in metres; the caller keeps phi in this pole's hemisphere (or accepts the far side's large rho) */
POLAR_HD void
polar_forward(const PolarProj &p, double phi, double lam, double &E, double &N)
{
	const double rho = p.scale * polar_t(p.pole > 0 ? phi : -phi), d = lam - p.lon0;
	E = rho * sin(d);
	N = p.pole > 0 ? -rho * cos(d) : rho * cos(d);
}

/* (E, N) to (phi, lam) in radians; lam is not wrapped */
POLAR_HD void
polar_inverse(const PolarProj &p, double E, double N, double &phi, double &lam)
{
	const double e = sqrt(POLAR_E2), rho = hypot(E, N), t = rho / p.scale;
	double f = POLAR_PI / 2.0 - 2.0 * atan(t);
	for (int it = 0; it < POLAR_INV_MAX; it++) {
		const double es = e * sin(f), next = POLAR_PI / 2.0 - 2.0 * atan(t * pow((1.0 - es) / (1.0 + es), e / 2.0));
		const double change = fabs(next - f);
		f = next;
		if (change < POLAR_INV_TOL) break;
	}
	phi = p.pole > 0 ? f : -f;
	lam = rho == 0.0 ? p.lon0 : p.lon0 + (p.pole > 0 ? atan2(E, -N) : atan2(E, N));
}

#endif
