"""
The reference's regression problems written against the pyclaw_amd surface, the way the
reference scripts are written against pyclaw (test/euler/2d/shockbubble.py,
test/acoustics/2d/homogeneous/acoustics.py, test/acoustics/1d/homogeneous/acoustics.py,
apps/advection/1d/constant/advection.py).  Shared by the GPU tests, smoke() and bench.py.
"""
import numpy as np

gamma = 1.4
gamma1 = gamma - 1.


def shock_state(pinf=5.):
    rinf = (gamma1 + pinf * (gamma + 1.)) / ((gamma + 1.) + gamma1 * pinf)
    vinf = 1. / np.sqrt(gamma) * (pinf - 1.) / np.sqrt(0.5 * ((gamma + 1.) / gamma) * pinf + 0.5 * gamma1 / gamma)
    einf = 0.5 * rinf * vinf ** 2 + pinf / gamma1
    return rinf, vinf, einf


def sb_qinit(state, x0=0.5, y0=0., r0=0.2, rhoin=0.1, pinf=5.):
    grid = state.grid
    rhoout = 1.
    pout = 1.
    pin = 1.
    x = grid.x.center
    y = grid.y.center
    Y, X = np.meshgrid(y, x)
    r = np.sqrt((X - x0) ** 2 + (Y - y0) ** 2)
    state.q[0, :, :] = rhoin * (r <= r0) + rhoout * (r > r0)
    state.q[1, :, :] = 0.
    state.q[2, :, :] = 0.
    state.q[3, :, :] = (pin * (r <= r0) + pout * (r > r0)) / gamma1
    state.q[4, :, :] = 1. * (r <= r0)


def sb_auxinit(state):
    y = state.grid.y.center
    for j, ycoord in enumerate(y):
        state.aux[0, :, j] = ycoord


def shockbc(state, dim, t, qbc, mbc):
    if dim.nstart == 0:
        rinf, vinf, einf = shock_state()
        for i in range(mbc):
            qbc[0, i, ...] = rinf
            qbc[1, i, ...] = rinf * vinf
            qbc[2, i, ...] = 0.
            qbc[3, i, ...] = einf
            qbc[4, i, ...] = 0.


def euler_rad_src(solver, state, dt):
    dt2 = dt / 2.
    ndim = 2
    aux = state.aux
    q = state.q
    rad = aux[0, :, :]
    rho = q[0, :, :]
    u = q[1, :, :] / rho
    v = q[2, :, :] / rho
    press = gamma1 * (q[3, :, :] - 0.5 * rho * (u ** 2 + v ** 2))
    qstar = np.empty(q.shape)
    qstar[0, :, :] = q[0, :, :] - dt2 * (ndim - 1) / rad * q[2, :, :]
    qstar[1, :, :] = q[1, :, :] - dt2 * (ndim - 1) / rad * rho * u * v
    qstar[2, :, :] = q[2, :, :] - dt2 * (ndim - 1) / rad * rho * v * v
    qstar[3, :, :] = q[3, :, :] - dt2 * (ndim - 1) / rad * v * (q[3, :, :] + press)
    rho = qstar[0, :, :]
    u = qstar[1, :, :] / rho
    v = qstar[2, :, :] / rho
    press = gamma1 * (qstar[3, :, :] - 0.5 * rho * (u ** 2 + v ** 2))
    q[0, :, :] = q[0, :, :] - dt * (ndim - 1) / rad * qstar[2, :, :]
    q[1, :, :] = q[1, :, :] - dt * (ndim - 1) / rad * rho * u * v
    q[2, :, :] = q[2, :, :] - dt * (ndim - 1) / rad * rho * v * v
    q[3, :, :] = q[3, :, :] - dt * (ndim - 1) / rad * v * (qstar[3, :, :] + press)


def dq_euler_radial(solver, state, dt):
    """apps/euler/2d/shockbubble/shockbubble.py:95-122 (dq_Euler_radial): the SharpClaw form of the source."""
    ndim = 2
    q = state.q
    rad = state.aux[0, :, :]
    rho = q[0, :, :]
    u = q[1, :, :] / rho
    v = q[2, :, :] / rho
    press = gamma1 * (q[3, :, :] - 0.5 * rho * (u ** 2 + v ** 2))
    dq = np.empty(q.shape)
    dq[0, :, :] = -dt * (ndim - 1) / rad * q[2, :, :]
    dq[1, :, :] = -dt * (ndim - 1) / rad * rho * u * v
    dq[2, :, :] = -dt * (ndim - 1) / rad * rho * v * v
    dq[3, :, :] = -dt * (ndim - 1) / rad * v * (q[3, :, :] + press)
    dq[4, :, :] = 0
    return dq


# The two callbacks above for ONE cell, as cell-function bodies (pyclaw.CellSource / pyclaw.CellDqSource): the same
# expressions in the same order, so that the 'exact' arithmetic gives the same bits.  p[0] = gamma1, p[1] = ndim.
EULER_RAD_CELL_SRC = """
const double gamma1 = p[0], ndm1 = p[1] - 1.0, dt = c.dt, dt2 = dt / 2., rad = aux[0];
double rho = q[0], u = q[1] / rho, v = q[2] / rho;
double press = gamma1 * (q[3] - 0.5 * rho * (u * u + v * v));
const double s0 = q[0] - dt2 * ndm1 / rad * q[2];
const double s1 = q[1] - dt2 * ndm1 / rad * rho * u * v;
const double s2 = q[2] - dt2 * ndm1 / rad * rho * v * v;
const double s3 = q[3] - dt2 * ndm1 / rad * v * (q[3] + press);
rho = s0; u = s1 / rho; v = s2 / rho;
press = gamma1 * (s3 - 0.5 * rho * (u * u + v * v));
q[0] = q[0] - dt * ndm1 / rad * s2;
q[1] = q[1] - dt * ndm1 / rad * rho * u * v;
q[2] = q[2] - dt * ndm1 / rad * rho * v * v;
q[3] = q[3] - dt * ndm1 / rad * v * (s3 + press);
"""

DQ_EULER_RAD_CELL_SRC = """
const double gamma1 = p[0], ndm1 = p[1] - 1.0, dt = c.dt, rad = aux[0];
const double rho = q[0], u = q[1] / rho, v = q[2] / rho;
const double press = gamma1 * (q[3] - 0.5 * rho * (u * u + v * v));
dq[0] = -dt * ndm1 / rad * q[2];
dq[1] = -dt * ndm1 / rad * rho * u * v;
dq[2] = -dt * ndm1 / rad * rho * v * v;
dq[3] = -dt * ndm1 / rad * v * (q[3] + press);
dq[4] = 0;
"""


# Normal Riemann solvers as bodies for pyclaw.CellRiemann: ql, qr, p[8] and the constant ixy in; wave, s, amdq, apdq out
# (zero on entry).  The first four restate built-in solvers expression by expression (pyclaw_amd/csrc/rp.hpp), so that
# the 'exact' arithmetic gives the bits of the built-in path; their p[] is the built-in solver's cparam.
ACOUSTICS_1D_RP = """
const double cc = p[2], zz = p[3];
const double d1 = qr[0] - ql[0];
const double d2 = qr[1] - ql[1];
const double a1 = (-d1 + zz * d2) / (2.0 * zz);
const double a2 = (d1 + zz * d2) / (2.0 * zz);
wave[0][0] = -a1 * zz; wave[0][1] = a1; s[0] = -cc;
wave[1][0] = a2 * zz;  wave[1][1] = a2; s[1] = cc;
for (int m = 0; m < 2; m++) { amdq[m] = s[0] * wave[0][m]; apdq[m] = s[1] * wave[1][m]; }
"""

# Burgers' equation with the transonic entropy fix
BURGERS_1D_RP = """
wave[0][0] = qr[0] - ql[0];
s[0] = 0.5 * (ql[0] + qr[0]);
const bool transonic = qr[0] > 0.0 && ql[0] < 0.0;
amdq[0] = transonic ? -0.5 * (ql[0] * ql[0]) : dmin(s[0], 0.0) * wave[0][0];
apdq[0] = transonic ? 0.5 * (qr[0] * qr[0]) : dmax(s[0], 0.0) * wave[0][0];
"""

# p = u, v
ADVECTION_2D_RP = """
const double vel = p[ixy - 1];
wave[0][0] = qr[0] - ql[0];
s[0] = vel;
amdq[0] = dmin(vel, 0.0) * wave[0][0];
apdq[0] = dmax(vel, 0.0) * wave[0][0];
"""

# q = (p, u, v); p = rho, bulk, cc, zz.  The transverse velocity's wave components stay the zeros they are on entry.
ACOUSTICS_2D_RP = """
constexpr int mu = (ixy == 1) ? 1 : 2;
const double cc = p[2], zz = p[3];
const double d1 = qr[0] - ql[0];
const double d2 = qr[mu] - ql[mu];
const double a1 = (-d1 + zz * d2) / (2.0 * zz);
const double a2 = (d1 + zz * d2) / (2.0 * zz);
wave[0][0] = -a1 * zz; wave[0][mu] = a1; s[0] = -cc;
wave[1][0] = a2 * zz;  wave[1][mu] = a2; s[1] = cc;
for (int m = 0; m < 3; m++) { amdq[m] = s[0] * wave[0][m]; apdq[m] = s[1] * wave[1][m]; }
"""

# A system the library does not have: scalar 2-D Burgers, q_t + (q^2/2)_x + (q^2/2)_y = 0 -- the 1-D body either way
BURGERS_2D_RP = BURGERS_1D_RP

# Solvers with cell-wise coefficients: pyclaw.CellRiemann(..., aux=...) hands the body auxl[], auxr[], the listed aux
# components of the cells left and right of the interface.  The first three restate the built-in solvers with aux
# (AdvectionColor1D, VcAdvection2D, VcAcoustics2D of pyclaw_amd/csrc/rp.hpp) expression by expression.

# colour equation q_t + u(x) q_x = 0, aux = (0,): the velocity at the cell's LEFT edge, so the interface takes auxr
ADVECTION_COLOR_1D_RP = """
wave[0][0] = qr[0] - ql[0];
s[0] = auxr[0];
amdq[0] = dmin(auxr[0], 0.0) * wave[0][0];
apdq[0] = dmax(auxr[0], 0.0) * wave[0][0];
"""

# 2-D colour equation, aux = (0, 1): u at the left edge, v at the bottom edge; the sweep direction picks one
VC_ADVECTION_2D_RP = """
const double vel = ixy == 1 ? auxr[0] : auxr[1];
wave[0][0] = qr[0] - ql[0];
s[0] = vel;
amdq[0] = dmin(vel, 0.0) * wave[0][0];
apdq[0] = dmax(vel, 0.0) * wave[0][0];
"""

# 2-D acoustics q = (p, u, v) with impedance and sound speed per cell, aux = (0, 1) = (Z, c); Z, c > 0
VC_ACOUSTICS_2D_RP = """
constexpr int mu = (ixy == 1) ? 1 : 2;
const double d1 = qr[0] - ql[0];
const double d2 = qr[mu] - ql[mu];
const double zi = auxr[0], zim = auxl[0];
const Recip by_zz(zim + zi);
const double a1 = by_zz.div(-d1 + zi * d2);
const double a2 = by_zz.div(d1 + zim * d2);
wave[0][0] = -a1 * zim; wave[0][mu] = a1; s[0] = -auxl[1];
wave[1][0] = a2 * zi;   wave[1][mu] = a2; s[1] = auxr[1];
amdq[0] = s[0] * wave[0][0]; amdq[mu] = s[0] * wave[0][mu];
apdq[0] = s[1] * wave[1][0]; apdq[mu] = s[1] * wave[1][mu];
"""

# A solver the library does not have: 1-D acoustics q = (p, u) in a layered medium, aux = (0, 1) = (Z, c) per cell
# (Clawpack's rp1_acoustics_variable): the left-going wave travels in the left cell, the right-going one in the right
VC_ACOUSTICS_1D_RP = """
const double d1 = qr[0] - ql[0];
const double d2 = qr[1] - ql[1];
const double zi = auxr[0], zim = auxl[0];
const double a1 = (-d1 + zi * d2) / (zim + zi);
const double a2 = (d1 + zim * d2) / (zim + zi);
wave[0][0] = -a1 * zim; wave[0][1] = a1; s[0] = -auxl[1];
wave[1][0] = a2 * zi;   wave[1][1] = a2; s[1] = auxr[1];
for (int m = 0; m < 2; m++) { amdq[m] = s[0] * wave[0][m]; apdq[m] = s[1] * wave[1][m]; }
"""

# Bodies for pyclaw.CellRiemann3D, the dimension-split 3-D step: ixy is 1, 2 or 3.

# 3-D acoustics q = (p, u, v, w) with impedance and sound speed per cell, aux = (0, 1) = (Z, c): the built-in
# vc_acoustics_3d (VcAcoustics3D of pyclaw_amd/csrc/rp.hpp) expression by expression
VC_ACOUSTICS_3D_RP = """
constexpr int mu = ixy;
const double d1 = qr[0] - ql[0];
const double d2 = qr[mu] - ql[mu];
const double zi = auxr[0], zim = auxl[0];
const Recip by_zz(zim + zi);
const double a1 = by_zz.div(-d1 + zi * d2);
const double a2 = by_zz.div(d1 + zim * d2);
wave[0][0] = -a1 * zim; wave[0][mu] = a1; s[0] = -auxl[1];
wave[1][0] = a2 * zi;   wave[1][mu] = a2; s[1] = auxr[1];
amdq[0] = s[0] * wave[0][0]; amdq[mu] = s[0] * wave[0][mu];
apdq[0] = s[1] * wave[1][0]; apdq[mu] = s[1] * wave[1][mu];
"""

# A solver the library does not have: 3-D acoustics in a homogeneous medium, no aux arrays; p = Z, c.  The formulas of the
# body above with both cells' coefficients taken from p[]: where the aux arrays of vc_acoustics_3d are constant, its bits
ACOUSTICS_3D_RP = """
constexpr int mu = ixy;
const double d1 = qr[0] - ql[0];
const double d2 = qr[mu] - ql[mu];
const double zz = p[0], cc = p[1];
const Recip by_zz(zz + zz);
const double a1 = by_zz.div(-d1 + zz * d2);
const double a2 = by_zz.div(d1 + zz * d2);
wave[0][0] = -a1 * zz; wave[0][mu] = a1; s[0] = -cc;
wave[1][0] = a2 * zz;  wave[1][mu] = a2; s[1] = cc;
amdq[0] = s[0] * wave[0][0]; amdq[mu] = s[0] * wave[0][mu];
apdq[0] = s[1] * wave[1][0]; apdq[mu] = s[1] * wave[1][mu];
"""

# p = u, v, w: the text of the 2-D body, the sweep direction picks the velocity
ADVECTION_3D_RP = ADVECTION_2D_RP

# scalar 3-D Burgers, q_t + (q^2/2)_x + (q^2/2)_y + (q^2/2)_z = 0 -- the 1-D body in every direction
BURGERS_3D_RP = BURGERS_1D_RP

# 3-D Euler equations, q = (rho, rho u, rho v, rho w, E), p = gamma: Roe solver with three waves (u - c, u, u + c; the
# middle one carries the entropy wave and both shear waves), no entropy fix.  Written in the sweep's own frame -- mu the
# normal momentum, mv and mw the other two in cyclic order -- so that a cyclic permutation of the axes and of the
# momentum components permutes the result bit for bit.
EULER_3D_RP = """
constexpr int mu = ixy, mv = ixy % 3 + 1, mw = (ixy + 1) % 3 + 1;
const double gamma1 = p[0] - 1.0;
const double rsl = dsqrt(ql[0]), rsr = dsqrt(qr[0]), rsq2 = rsl + rsr;
const double pl = gamma1 * (ql[4] - 0.5 * (ql[mu] * ql[mu] + ql[mv] * ql[mv] + ql[mw] * ql[mw]) / ql[0]);
const double pr = gamma1 * (qr[4] - 0.5 * (qr[mu] * qr[mu] + qr[mv] * qr[mv] + qr[mw] * qr[mw]) / qr[0]);
const double u = (ql[mu] / rsl + qr[mu] / rsr) / rsq2;
const double v = (ql[mv] / rsl + qr[mv] / rsr) / rsq2;
const double w = (ql[mw] / rsl + qr[mw] / rsr) / rsq2;
const double enth = ((ql[4] + pl) / rsl + (qr[4] + pr) / rsr) / rsq2;
const double uvw2 = u * u + v * v + w * w;
const double a2 = gamma1 * (enth - 0.5 * uvw2);
const double a = dsqrt(a2);
const double g1a2 = gamma1 / a2, euv = enth - uvw2;
const double d1 = qr[0] - ql[0], d2 = qr[mu] - ql[mu], d3 = qr[mv] - ql[mv], d4 = qr[mw] - ql[mw], d5 = qr[4] - ql[4];
const double b4 = g1a2 * (euv * d1 + u * d2 + v * d3 + w * d4 - d5);
const double b2 = d3 - v * d1;
const double b3 = d4 - w * d1;
const double b5 = (d2 + (a - u) * d1 - a * b4) / (2.0 * a);
const double b1 = d1 - b4 - b5;
wave[0][0] = b1; wave[0][mu] = b1 * (u - a); wave[0][mv] = b1 * v; wave[0][mw] = b1 * w; wave[0][4] = b1 * (enth - u * a);
s[0] = u - a;
wave[1][0] = b4; wave[1][mu] = b4 * u; wave[1][mv] = b4 * v + b2; wave[1][mw] = b4 * w + b3;
wave[1][4] = b4 * 0.5 * uvw2 + b2 * v + b3 * w;
s[1] = u;
wave[2][0] = b5; wave[2][mu] = b5 * (u + a); wave[2][mv] = b5 * v; wave[2][mw] = b5 * w; wave[2][4] = b5 * (enth + u * a);
s[2] = u + a;
for (int m = 0; m < 5; m++) {
    amdq[m] = dmin(s[0], 0.0) * wave[0][m] + dmin(s[1], 0.0) * wave[1][m] + dmin(s[2], 0.0) * wave[2][m];
    apdq[m] = dmax(s[0], 0.0) * wave[0][m] + dmax(s[1], 0.0) * wave[1][m] + dmax(s[2], 0.0) * wave[2][m];
}
"""

# Transverse bodies for pyclaw.CellRiemann3D(..., rpt3=..., rptt3=...), the unsplit 3-D step: ixyz is the direction of the
# normal solve, icoor 2 / 3 the y-like / z-like direction the split is made in, so the split direction (1-based, cyclic) is
_SPLIT_DIR_3D = "constexpr int iuvw = (ixyz + icoor - 2) % 3 + 1;"

# The built-in vc_acoustics_3d's transverse solvers (rpt3_vc_acoustics / rptt3_vc_acoustics of oracle/classic_oracle.c)
# expression by expression, in general form: the velocity component of the split direction takes part in a1 and a2 even
# where the library's own kernel knows it to be zero.  aux = (0, 1) = (Z, c); auxb[a][b][k] is the neighbour at y-like
# offset a-1, z-like offset b-1.  The part going down enters the neighbouring row with ITS impedance and sound speed.
VC_ACOUSTICS_3D_RPT = _SPLIT_DIR_3D + """
const double zm = icoor == 2 ? auxb[0][1][0] : auxb[1][0][0], zz = auxb[1][1][0], zp = icoor == 2 ? auxb[2][1][0] : auxb[1][2][0];
const double cm = icoor == 2 ? auxb[0][1][1] : auxb[1][0][1], cp = icoor == 2 ? auxb[2][1][1] : auxb[1][2][1];
const double a1 = fdiv(-asdq[0] + asdq[iuvw] * zz, zm + zz);
const double a2 = fdiv(asdq[0] + asdq[iuvw] * zz, zz + zp);
bmasdq[0] = cm * a1 * zm; bmasdq[iuvw] = -cm * a1;
bpasdq[0] = cp * a2 * zp; bpasdq[iuvw] = cp * a2;
"""
# the new split lies inside the row the input went to: the z-like row impt names (icoor 2) or the y-like one (icoor 3)
VC_ACOUSTICS_3D_RPTT = _SPLIT_DIR_3D + """
const int r = impt == 1 ? 0 : 2;
const double zm = icoor == 2 ? auxb[0][r][0] : auxb[r][0][0], zz = icoor == 2 ? auxb[1][r][0] : auxb[r][1][0];
const double zp = icoor == 2 ? auxb[2][r][0] : auxb[r][2][0];
const double cm = icoor == 2 ? auxb[0][r][1] : auxb[r][0][1], cp = icoor == 2 ? auxb[2][r][1] : auxb[r][2][1];
const double a1 = fdiv(-bsasdq[0] + bsasdq[iuvw] * zz, zm + zz);
const double a2 = fdiv(bsasdq[0] + bsasdq[iuvw] * zz, zz + zp);
cmbsasdq[0] = cm * a1 * zm; cmbsasdq[iuvw] = -cm * a1;
cpbsasdq[0] = cp * a2 * zp; cpbsasdq[iuvw] = cp * a2;
"""

# homogeneous 3-D acoustics, no aux arrays; p = Z, c: the two bodies above with every coefficient taken from p[]
ACOUSTICS_3D_RPT = _SPLIT_DIR_3D + """
const double zz = p[0], cc = p[1];
const double a1 = fdiv(-asdq[0] + asdq[iuvw] * zz, zz + zz);
const double a2 = fdiv(asdq[0] + asdq[iuvw] * zz, zz + zz);
bmasdq[0] = cc * a1 * zz; bmasdq[iuvw] = -cc * a1;
bpasdq[0] = cc * a2 * zz; bpasdq[iuvw] = cc * a2;
"""
ACOUSTICS_3D_RPTT = _SPLIT_DIR_3D + """
const double zz = p[0], cc = p[1];
const double a1 = fdiv(-bsasdq[0] + bsasdq[iuvw] * zz, zz + zz);
const double a2 = fdiv(bsasdq[0] + bsasdq[iuvw] * zz, zz + zz);
cmbsasdq[0] = cc * a1 * zz; cmbsasdq[iuvw] = -cc * a1;
cpbsasdq[0] = cc * a2 * zz; cpbsasdq[iuvw] = cc * a2;
"""

# p = u, v, w: the part of the input moving down / up with the velocity of the split direction
ADVECTION_3D_RPT = _SPLIT_DIR_3D + """
const double vel = p[iuvw - 1];
bmasdq[0] = dmin(vel, 0.0) * asdq[0];
bpasdq[0] = dmax(vel, 0.0) * asdq[0];
"""
ADVECTION_3D_RPTT = _SPLIT_DIR_3D + """
const double vel = p[iuvw - 1];
cmbsasdq[0] = dmin(vel, 0.0) * bsasdq[0];
cpbsasdq[0] = dmax(vel, 0.0) * bsasdq[0];
"""

# 3-D Euler: the three-wave Roe decomposition of EULER_3D_RP in the frame of the split direction -- mu its momentum, mv
# and mw the other two in cyclic order -- with the Roe averages of ql and qr, applied to the input in place of qr - ql;
# the parts with negative speeds go down, those with positive speeds up.  IN_, OM_, OP_ stand for the three arrays.
_EULER_3D_SPLIT = _SPLIT_DIR_3D + """
constexpr int mu = iuvw, mv = iuvw % 3 + 1, mw = (iuvw + 1) % 3 + 1;
const double gamma1 = p[0] - 1.0;
const double rsl = dsqrt(ql[0]), rsr = dsqrt(qr[0]), rsq2 = rsl + rsr;
const double pl = gamma1 * (ql[4] - 0.5 * (ql[mu] * ql[mu] + ql[mv] * ql[mv] + ql[mw] * ql[mw]) / ql[0]);
const double pr = gamma1 * (qr[4] - 0.5 * (qr[mu] * qr[mu] + qr[mv] * qr[mv] + qr[mw] * qr[mw]) / qr[0]);
const double u = (ql[mu] / rsl + qr[mu] / rsr) / rsq2;
const double v = (ql[mv] / rsl + qr[mv] / rsr) / rsq2;
const double w = (ql[mw] / rsl + qr[mw] / rsr) / rsq2;
const double enth = ((ql[4] + pl) / rsl + (qr[4] + pr) / rsr) / rsq2;
const double uvw2 = u * u + v * v + w * w;
const double a2 = gamma1 * (enth - 0.5 * uvw2);
const double a = dsqrt(a2);
const double g1a2 = gamma1 / a2, euv = enth - uvw2;
const double d1 = IN_[0], d2 = IN_[mu], d3 = IN_[mv], d4 = IN_[mw], d5 = IN_[4];
const double b4 = g1a2 * (euv * d1 + u * d2 + v * d3 + w * d4 - d5);
const double b2 = d3 - v * d1;
const double b3 = d4 - w * d1;
const double b5 = (d2 + (a - u) * d1 - a * b4) / (2.0 * a);
const double b1 = d1 - b4 - b5;
double w0[5], w1[5], w2[5];
w0[0] = b1; w0[mu] = b1 * (u - a); w0[mv] = b1 * v; w0[mw] = b1 * w; w0[4] = b1 * (enth - u * a);
w1[0] = b4; w1[mu] = b4 * u; w1[mv] = b4 * v + b2; w1[mw] = b4 * w + b3; w1[4] = b4 * 0.5 * uvw2 + b2 * v + b3 * w;
w2[0] = b5; w2[mu] = b5 * (u + a); w2[mv] = b5 * v; w2[mw] = b5 * w; w2[4] = b5 * (enth + u * a);
const double s0 = u - a, s1 = u, s2 = u + a;
for (int m = 0; m < 5; m++) {
    OM_[m] = dmin(s0, 0.0) * w0[m] + dmin(s1, 0.0) * w1[m] + dmin(s2, 0.0) * w2[m];
    OP_[m] = dmax(s0, 0.0) * w0[m] + dmax(s1, 0.0) * w1[m] + dmax(s2, 0.0) * w2[m];
}
"""
EULER_3D_RPT = _EULER_3D_SPLIT.replace("IN_", "asdq").replace("OM_", "bmasdq").replace("OP_", "bpasdq")
EULER_3D_RPTT = _EULER_3D_SPLIT.replace("IN_", "bsasdq").replace("OM_", "cmbsasdq").replace("OP_", "cpbsasdq")

# F-wave solvers: pyclaw.CellRiemann(..., fwave=True) with solver.fwave = True.  The array the body assigns is fwave[][],
# the pieces of the flux difference; between two EQUAL cells over different coefficients they are not zero, and every
# interface is solved.

# 1-D nonlinear elasticity in a layered medium, q = (eps, rho u), aux = (0, 1, 2) = (rho, K, stress-law flag): the
# arithmetic of the built-in elasticity_fwave_1d (FwaveElastic<2> of rp.hpp: its precell of either cell, then its solve)
# in its operation order.  ps_sigma / ps_sigmap are rp.hpp's: flag 1 is sigma = K eps, anything else exp(K eps) - 1.
ELASTICITY_FWAVE_1D_RP = """
const double rhol = auxl[0], rhor = auxr[0];
const double unl = fdiv_ieee(ql[1], rhol), unr = fdiv_ieee(qr[1], rhor);
const double sigl = ps_sigma(ql[0], auxl[1], auxl[2]), sigr = ps_sigma(qr[0], auxr[1], auxr[2]);
const double cl = dsqrt(fdiv_ieee(ps_sigmap(ql[0], auxl[1], auxl[2]), rhol));
const double cr = dsqrt(fdiv_ieee(ps_sigmap(qr[0], auxr[1], auxr[2]), rhor));
const double zl = cl * rhol, zr = cr * rhor;
const double du = unr - unl;
const double dsig = sigr - sigl;
const double zs = zl + zr;
const double b1 = fdiv_ieee(-(zr * du + dsig), zs);
const double b2 = fdiv_ieee(-(zl * du - dsig), zs);
fwave[0][0] = b1; fwave[0][1] = b1 * zl; s[0] = -cl;
fwave[1][0] = b2; fwave[1][1] = b2 * (-zr); s[1] = cr;
for (int m = 0; m < 2; m++) { amdq[m] = fwave[0][m]; apdq[m] = fwave[1][m]; }
"""

# A solver the library does not have: conservative advection with a variable speed, q_t + (u(x) q)_x = 0, aux = (0,) =
# u at the cell centre.  One f-wave, the flux difference itself; between equal cells it is (ur - ul) q, not zero.
VC_ADVECTION_FWAVE_1D_RP = """
const double ul = auxl[0], ur = auxr[0];
fwave[0][0] = ur * qr[0] - ul * ql[0];
s[0] = 0.5 * (ul + ur);
if (s[0] >= 0.0) apdq[0] = fwave[0][0];
else amdq[0] = fwave[0][0];
"""

# A solver the library does not have: 1-D shallow water over bathymetry, q = (h, hu), aux = (0,) = b, p = g.  Roe-type
# speeds; the flux difference takes the source term g h b_x with it as g * (hl + hr)/2 * (br - bl) and is decomposed on the
# eigenvectors (1, s0), (1, s1): a lake at rest (hu = 0, h + b constant) has f-waves that are zero, so it stays at rest --
# the well-balanced solver people write f-wave solvers for.  h > 0.
SHALLOW_BATHY_FWAVE_1D_RP = """
const double g = p[0];
const double hl = ql[0], hr = qr[0];
const double ul = ql[1] / hl, ur = qr[1] / hr;
const double hbar = 0.5 * (hl + hr);
const double rl = dsqrt(hl), rr = dsqrt(hr);
const double uhat = (rl * ul + rr * ur) / (rl + rr);
const double chat = dsqrt(g * hbar);
s[0] = uhat - chat; s[1] = uhat + chat;
const double d0 = qr[1] - ql[1];
const double d1 = (qr[1] * ur + 0.5 * g * hr * hr) - (ql[1] * ul + 0.5 * g * hl * hl) + g * hbar * (auxr[0] - auxl[0]);
const double b1 = (s[1] * d0 - d1) / (s[1] - s[0]);
const double b2 = (d1 - s[0] * d0) / (s[1] - s[0]);
fwave[0][0] = b1; fwave[0][1] = b1 * s[0];
fwave[1][0] = b2; fwave[1][1] = b2 * s[1];
for (int mw = 0; mw < 2; mw++)
    for (int m = 0; m < 2; m++) {
        if (s[mw] < 0.0) amdq[m] += fwave[mw][m];
        else apdq[m] += fwave[mw][m];
    }
"""

# Transverse Riemann solvers as bodies for pyclaw.CellRiemann(..., transverse=...): Clawpack's rpt2 for one interface, for
# the unsplit step.  ixy is the direction of the NORMAL solve, asdq the fluctuation to split, bmasdq / bpasdq (zero on
# entry) its down- and up-going parts.  Without aux the body sees ql, qr; with aux q1, aux1 (the cell asdq belongs to)
# and aux_below, aux_above.  The first five restate the built-in transverse solvers of rp.hpp in their operation order.

# p = u, v: the velocity across the sweep
ADVECTION_2D_RPT = """
const double stran = p[2 - ixy];
bmasdq[0] = dmin(stran, 0.0) * asdq[0];
bpasdq[0] = dmax(stran, 0.0) * asdq[0];
"""

# (the normal velocity's components stay the zeros they are on entry)
ACOUSTICS_2D_RPT = """
constexpr int mv = (ixy == 1) ? 2 : 1;
const double cc = p[2], zz = p[3];
const double a1 = (-asdq[0] + zz * asdq[mv]) / (2.0 * zz);
const double a2 = (asdq[0] + zz * asdq[mv]) / (2.0 * zz);
bmasdq[0] = cc * a1 * zz; bmasdq[mv] = -cc * a1;
bpasdq[0] = cc * a2 * zz; bpasdq[mv] = cc * a2;
"""

# aux = (0, 1) = (Z, c): the down-going part enters the slice below with that slice's impedance and sound speed, the
# up-going part the slice above
VC_ACOUSTICS_2D_RPT = """
constexpr int mv = (ixy == 1) ? 2 : 1;
const double zm = aux_below[0], zz = aux1[0], zp = aux_above[0], cm = aux_below[1], cp = aux_above[1];
const double a1 = fdiv_ieee(-asdq[0] + asdq[mv] * zz, zm + zz);
const double a2 = fdiv_ieee(asdq[0] + asdq[mv] * zz, zz + zp);
bmasdq[0] = cm * a1 * zm; bmasdq[mv] = -cm * a1;
bpasdq[0] = cp * a2 * zp; bpasdq[mv] = cp * a2;
"""

# aux = (0, 1): u at the left edge, v at the bottom edge.  Down-going: the transverse velocity at the cell's own lower
# edge; up-going: at the lower edge of the cell above
VC_ADVECTION_2D_RPT = """
const double own = ixy == 1 ? aux1[1] : aux1[0], above = ixy == 1 ? aux_above[1] : aux_above[0];
bmasdq[0] = dmin(own, 0.0) * asdq[0];
bpasdq[0] = dmax(above, 0.0) * asdq[0];
"""

# 2-D shallow water q = (h, hu, hv), p = g: Roe solver with the Harten-Hyman entropy fix (Shallow2D of rp.hpp) and its
# transverse solver, which splits with the Roe average of the interface's two cells: the one that needs ql and qr
SHALLOW_2D_RP = """
constexpr int mu = (ixy == 1) ? 1 : 2, mv = (ixy == 1) ? 2 : 1;
const double g = p[0];
const double rh = (ql[0] + qr[0]) * 0.5;
const double hsl = dsqrt(ql[0]), hsr = dsqrt(qr[0]), hsq2 = hsl + hsr;
const double ru = (ql[mu] / hsl + qr[mu] / hsr) / hsq2;
const double rv = (ql[mv] / hsl + qr[mv] / hsr) / hsq2;
const double ra = dsqrt(g * rh);
const double d1 = qr[0] - ql[0], d2 = qr[mu] - ql[mu], d3 = qr[mv] - ql[mv];
const double a1 = ((ru + ra) * d1 - d2) * (0.5 / ra);
const double a2 = -rv * d1 + d3;
const double a3 = (-(ru - ra) * d1 + d2) * (0.5 / ra);
wave[0][0] = a1;  wave[0][mu] = a1 * (ru - ra); wave[0][mv] = a1 * rv; s[0] = ru - ra;
wave[1][0] = 0.0; wave[1][mu] = 0.0;            wave[1][mv] = a2;      s[1] = ru;
wave[2][0] = a3;  wave[2][mu] = a3 * (ru + ra); wave[2][mv] = a3 * rv; s[2] = ru + ra;
const double hl = ql[0], hr = qr[0];
const double s0 = ql[mu] / hl - dsqrt(g * hl);
const bool all_right = (s0 >= 0.0) && (s[0] > 0.0);
{
    const double h1 = hl + wave[0][0], hu1 = ql[mu] + wave[0][mu];
    const double s1 = hu1 / h1 - dsqrt(g * h1);
    double sfract;
    if (s0 < 0.0 && s1 > 0.0) sfract = s0 * (s1 - s[0]) / (s1 - s0);
    else if (s[0] < 0.0) sfract = s[0];
    else sfract = 0.0;
    for (int m = 0; m < 3; m++) amdq[m] = sfract * wave[0][m];
}
if (!(s[1] >= 0.0)) {
    for (int m = 0; m < 3; m++) amdq[m] = amdq[m] + s[1] * wave[1][m];
    const double s03 = qr[mu] / hr + dsqrt(g * hr);
    const double h3 = hr - wave[2][0], hu3 = qr[mu] - wave[2][mu];
    const double s3 = hu3 / h3 + dsqrt(g * h3);
    double sfract = 0.0;
    bool add = true;
    if (s3 < 0.0 && s03 > 0.0) sfract = s3 * (s03 - s[2]) / (s03 - s3);
    else if (s[2] < 0.0) sfract = s[2];
    else add = false;
    if (add) for (int m = 0; m < 3; m++) amdq[m] = amdq[m] + sfract * wave[2][m];
}
if (all_right) for (int m = 0; m < 3; m++) amdq[m] = 0.0;
for (int m = 0; m < 3; m++) {
    double df = s[0] * wave[0][m];
    df = df + s[1] * wave[1][m];
    df = df + s[2] * wave[2][m];
    apdq[m] = df - amdq[m];
}
"""

SHALLOW_2D_RPT = """
constexpr int mu = (ixy == 1) ? 1 : 2, mv = (ixy == 1) ? 2 : 1;
const double rh = (ql[0] + qr[0]) * 0.5;
const double hsl = dsqrt(ql[0]), hsr = dsqrt(qr[0]), hsq2 = hsl + hsr;
const double ru = (ql[mu] / hsl + qr[mu] / hsr) / hsq2;
const double rv = (ql[mv] / hsl + qr[mv] / hsr) / hsq2;
const double ra = dsqrt(p[0] * rh);
const double a1 = (0.5 / ra) * ((rv + ra) * asdq[0] - asdq[mv]);
const double a2 = asdq[mu] - ru * asdq[0];
const double a3 = (0.5 / ra) * (-(rv - ra) * asdq[0] + asdq[mv]);
double wb[3][3], sb[3];
wb[0][0] = a1;  wb[0][mu] = a1 * ru; wb[0][mv] = a1 * (rv - ra); sb[0] = rv - ra;
wb[1][0] = 0.0; wb[1][mu] = a2;      wb[1][mv] = 0.0;            sb[1] = rv;
wb[2][0] = a3;  wb[2][mu] = a3 * ru; wb[2][mv] = a3 * (rv + ra); sb[2] = rv + ra;
for (int m = 0; m < 3; m++) {
    double m_ = 0.0, p_ = 0.0;
    for (int mw = 0; mw < 3; mw++) {
        m_ = m_ + dmin(sb[mw], 0.0) * wb[mw][m];
        p_ = p_ + dmax(sb[mw], 0.0) * wb[mw][m];
    }
    bmasdq[m] = m_; bpasdq[m] = p_;
}
"""

# MEQN independent advected scalars, mwaves = meqn <= 8: wave k carries component k alone, x velocity p[k], y velocity
# -p[k] / 2 (an exact scaling, so each component is advection_2d with those two velocities bit for bit).  The largest
# systems a CellRiemann takes: meqn = 7 and 8 run the unsplit kernels with 12 slices per workgroup.
SCALARS_2D_RP = """
for (int k = 0; k < MEQN; k++) {
    const double vel = ixy == 1 ? p[k] : -0.5 * p[k];
    wave[k][k] = qr[k] - ql[k];
    s[k] = vel;
    amdq[k] = dmin(vel, 0.0) * wave[k][k];
    apdq[k] = dmax(vel, 0.0) * wave[k][k];
}
"""

SCALARS_2D_RPT = """
for (int k = 0; k < MEQN; k++) {
    const double stran = ixy == 1 ? -0.5 * p[k] : p[k];
    bmasdq[k] = dmin(stran, 0.0) * asdq[k];
    bpasdq[k] = dmax(stran, 0.0) * asdq[k];
}
"""

# scalar 2-D Burgers (BURGERS_2D_RP): the transverse speed is the average of the interface's two cells
BURGERS_2D_RPT = """
const double sb = 0.5 * (ql[0] + qr[0]);
bmasdq[0] = dmin(sb, 0.0) * asdq[0];
bpasdq[0] = dmax(sb, 0.0) * asdq[0];
"""


def shockbubble(pyclaw, mx=160, my=40, tfinal=0.2, device_callbacks=False, with_src=True,
                dim_split=True, order_trans=2, dt_initial=0.005, nout=1, run=True, math='exact',
                solver_type='classic', time_integrator='SSP104'):
    """test/euler/2d/shockbubble.py:97-166; solver_type='sharpclaw' as in apps/euler/2d/shockbubble/shockbubble.py:173-176
    (dq_src in place of step_src, WENO5).  device_callbacks=True swaps the Python custom-BC / source callbacks for the
    built-in device versions (same arithmetic)."""
    x = pyclaw.Dimension('x', 0.0, 2.0, mx)
    y = pyclaw.Dimension('y', 0.0, 0.5, my)
    grid = pyclaw.Grid([x, y])
    meqn = 5
    maux = 1
    state = pyclaw.State(grid, meqn, maux)
    state.aux_global['gamma'] = gamma
    state.aux_global['gamma1'] = gamma1
    sb_qinit(state)
    sb_auxinit(state)
    initial_solution = pyclaw.Solution(state)

    sharp = solver_type == 'sharpclaw'
    solver = pyclaw.SharpClawSolver2D() if sharp else pyclaw.ClawSolver2D()
    solver.math = math
    solver.rp = pyclaw.riemann.rp_euler_5wave_2d
    solver.mwaves = 5
    solver.dt_initial = dt_initial
    if sharp:
        solver.weno_order = 5
        solver.lim_type = 2
        solver.time_integrator = time_integrator
    else:
        solver.cfl_max = 0.5
        solver.cfl_desired = 0.45
        solver.limiters = [4, 4, 4, 4, 2]
        solver.dim_split = dim_split
        solver.order_trans = order_trans
        solver.src_split = 1
    if device_callbacks:
        rinf, vinf, einf = shock_state()
        solver.user_bc_lower = pyclaw.ConstantStateBC([rinf, rinf * vinf, 0., einf, 0.])
        src = (pyclaw.EulerRadialDqSource if sharp else pyclaw.EulerRadialSource)(gamma1, 2)
    else:
        solver.user_bc_lower = shockbc
        src = dq_euler_radial if sharp else euler_rad_src
    if sharp:
        solver.dq_src = src if with_src else None
    else:
        solver.step_src = src if with_src else None
    solver.bc_lower[0] = pyclaw.BC.custom
    solver.bc_upper[0] = pyclaw.BC.outflow
    solver.bc_lower[1] = pyclaw.BC.reflecting
    solver.bc_upper[1] = pyclaw.BC.outflow
    solver.aux_bc_lower[0] = pyclaw.BC.outflow
    solver.aux_bc_upper[0] = pyclaw.BC.outflow
    solver.aux_bc_lower[1] = pyclaw.BC.outflow
    solver.aux_bc_upper[1] = pyclaw.BC.outflow

    claw = pyclaw.Controller()
    claw.keep_copy = True
    claw.tfinal = tfinal
    claw.solution = initial_solution
    claw.solver = solver
    claw.nout = nout
    if not run:
        return claw
    claw.run()
    return claw


def ac2d_qinit(state, width=0.2):
    grid = state.grid
    x = grid.x.center
    y = grid.y.center
    Y, X = np.meshgrid(y, x)
    r = np.sqrt(X ** 2 + Y ** 2)
    state.q[0, :, :] = (np.abs(r - 0.5) <= width) * (1. + np.cos(np.pi * (r - 0.5) / width))
    state.q[1, :, :] = 0.
    state.q[2, :, :] = 0.


def acoustics2D(pyclaw, mx=100, my=100, tfinal=0.12, nout=10, dim_split=1, run=True, math='exact',
                solver_type='classic', lim_type=2, time_integrator='SSP104', weno_order=5, user_rp=False):
    """test/acoustics/2d/homogeneous/acoustics.py:19-86 (classic or sharpclaw).  user_rp=True: the same solver as the
    bodies ACOUSTICS_2D_RP / ACOUSTICS_2D_RPT of a pyclaw.CellRiemann, dimension-split or unsplit (classic), or as
    ACOUSTICS_2D_RP compiled for the SharpClaw stages (sharpclaw=True)."""
    if solver_type == 'classic':
        solver = pyclaw.ClawSolver2D()
    else:
        solver = pyclaw.SharpClawSolver2D()
        solver.lim_type = lim_type
        solver.time_integrator = time_integrator
        solver.weno_order = weno_order
    solver.math = math
    solver.rp = pyclaw.riemann.rp_acoustics_2d
    solver.cfl_max = 0.5
    solver.cfl_desired = 0.45
    solver.mwaves = 2
    solver.dim_split = dim_split
    solver.limiters = [4] * solver.mwaves
    solver.bc_lower[0] = pyclaw.BC.outflow
    solver.bc_upper[0] = pyclaw.BC.outflow
    solver.bc_lower[1] = pyclaw.BC.outflow
    solver.bc_upper[1] = pyclaw.BC.outflow
    x = pyclaw.Dimension('x', -1.0, 1.0, mx)
    y = pyclaw.Dimension('y', -1.0, 1.0, my)
    grid = pyclaw.Grid([x, y])
    state = pyclaw.State(grid, 3)
    rho = 1.0
    bulk = 4.0
    cc = np.sqrt(bulk / rho)
    zz = rho * cc
    state.aux_global['rho'] = rho
    state.aux_global['bulk'] = bulk
    state.aux_global['zz'] = zz
    state.aux_global['cc'] = cc
    ac2d_qinit(state)
    if user_rp and solver_type != 'classic':
        solver.rp = pyclaw.CellRiemann(ACOUSTICS_2D_RP, 3, 2, 2, params=[rho, bulk, cc, zz], name="acoustics_2d_user",
                                       sharpclaw=True)
    elif user_rp:
        # (the transverse body only where the unsplit step asks for it: the split run compiles the two sweeps alone)
        solver.rp = pyclaw.CellRiemann(ACOUSTICS_2D_RP, 3, 2, 2, params=[rho, bulk, cc, zz], name="acoustics_2d_user",
                                       transverse=None if dim_split else ACOUSTICS_2D_RPT)
    initial_solution = pyclaw.Solution(state)
    solver.dt_initial = np.min(grid.d) / state.aux_global['cc'] * solver.cfl_desired
    claw = pyclaw.Controller()
    claw.keep_copy = True
    claw.tfinal = tfinal
    claw.solution = initial_solution
    claw.solver = solver
    claw.nout = nout
    if not run:
        return claw
    claw.run()
    return claw


def vc_acoustics2D(pyclaw, mx=100, my=100, tfinal=0.12, nout=10, run=True, math='exact', user_rp=False, dim_split=1):
    """The pulse of acoustics2D in a layered medium: impedance and sound speed per cell in aux(1), aux(2) -- four layers
    in x with the sound speeds 2, 1.5, 1, 1.25 and an impedance that also varies smoothly in y.  Dimension-split or
    unsplit (dim_split=0), with rp_vc_acoustics_2d or, user_rp=True, the same solver as the bodies VC_ACOUSTICS_2D_RP /
    VC_ACOUSTICS_2D_RPT of a pyclaw.CellRiemann."""
    claw = acoustics2D(pyclaw, mx=mx, my=my, tfinal=tfinal, nout=nout, run=False, math=math, dim_split=dim_split)
    old = claw.solution.state
    state = pyclaw.State(old.grid, 3, 2)
    state.q[...] = old.q
    X, Y = old.grid.c_center
    layer = np.minimum((2.0 * (X + 1.0)).astype(int), 3)
    cc = np.array([2.0, 1.5, 1.0, 1.25])[layer]
    state.aux[0] = cc * (1.0 + 0.25 * np.sin(np.pi * Y))       # Z = rho c with a density that varies in y
    state.aux[1] = cc
    claw.solution = pyclaw.Solution(state)
    solver = claw.solver
    solver.rp = (pyclaw.CellRiemann(VC_ACOUSTICS_2D_RP, 3, 2, 2, aux=(0, 1), name="vc_acoustics_2d_user",
                                    transverse=None if dim_split else VC_ACOUSTICS_2D_RPT) if user_rp
                 else pyclaw.riemann.rp_vc_acoustics_2d)
    for k in range(2):
        solver.aux_bc_lower[k] = solver.aux_bc_upper[k] = pyclaw.BC.outflow
    solver.dt_initial = np.min(old.grid.d) / 2.0 * solver.cfl_desired
    if run:
        claw.run()
    return claw


def capa_acoustics2D(pyclaw, mx=100, my=100, tfinal=0.12, nout=10, run=True, math='exact', user_rp=False, dim_split=1):
    """The pulse of acoustics2D on a grid with a smooth capacity function in aux(1), state.mcapa = 0 (the cell areas of a
    mapped grid, between 0.6 and 1.4): dimension-split or unsplit (dim_split=0), with rp_acoustics_2d or, user_rp=True,
    the bodies ACOUSTICS_2D_RP / ACOUSTICS_2D_RPT unchanged in a pyclaw.CellRiemann compiled with capa=True."""
    claw = acoustics2D(pyclaw, mx=mx, my=my, tfinal=tfinal, nout=nout, run=False, math=math, dim_split=dim_split)
    old = claw.solution.state
    state = pyclaw.State(old.grid, 3, 1)
    state.q[...] = old.q
    state.aux_global.update(old.aux_global)
    X, Y = old.grid.c_center
    state.aux[0] = 1.0 + 0.4 * np.sin(np.pi * X) * np.cos(0.5 * np.pi * Y)
    state.mcapa = 0
    claw.solution = pyclaw.Solution(state)
    solver = claw.solver
    if user_rp:
        g = state.aux_global
        solver.rp = pyclaw.CellRiemann(ACOUSTICS_2D_RP, 3, 2, 2, params=[g['rho'], g['bulk'], g['cc'], g['zz']], capa=True,
                                       name="acoustics_2d_capa_user", transverse=None if dim_split else ACOUSTICS_2D_RPT)
    for k in range(2):
        solver.aux_bc_lower[k] = solver.aux_bc_upper[k] = pyclaw.BC.outflow
    solver.dt_initial = 0.6 * solver.dt_initial       # the Courant number is dt / (dx capa) c, capa >= 0.6
    if run:
        claw.run()
    return claw


def acoustics1D(pyclaw, mx=100, solver_type='classic', lim_type=2, time_integrator='SSP104', weno_order=5,
                math='exact', char_decomp=0, user_rp=False, run=True):
    """test/acoustics/1d/homogeneous/acoustics.py: returns the one-period L1 error.  user_rp=True: the same solver as the
    body ACOUSTICS_1D_RP of a pyclaw.CellRiemann, compiled for the classic step or for the SharpClaw stages.  run=False:
    (None, the controller) before anything ran."""
    if solver_type == 'classic':
        solver = pyclaw.ClawSolver1D()
    else:
        solver = pyclaw.SharpClawSolver1D()
        solver.lim_type = lim_type
        solver.time_integrator = time_integrator
        solver.weno_order = weno_order
        solver.char_decomp = char_decomp
    solver.math = math
    solver.rp = pyclaw.riemann.rp_acoustics_1d
    x = pyclaw.Dimension('x', 0.0, 1.0, mx)
    grid = pyclaw.Grid(x)
    state = pyclaw.State(grid, 2)
    rho = 1.0
    bulk = 1.0
    state.aux_global['rho'] = rho
    state.aux_global['bulk'] = bulk
    state.aux_global['zz'] = np.sqrt(rho * bulk)
    state.aux_global['cc'] = np.sqrt(rho / bulk)
    if user_rp:
        g = state.aux_global
        solver.rp = pyclaw.CellRiemann(ACOUSTICS_1D_RP, 2, 2, 1, params=[g['rho'], g['bulk'], g['cc'], g['zz']],
                                       name="acoustics_1d_user", sharpclaw=solver_type != 'classic')
    xc = grid.x.center
    beta = 100
    gam = 0
    x0 = 0.75
    state.q[0, :] = np.exp(-beta * (xc - x0) ** 2) * np.cos(gam * (xc - x0))
    state.q[1, :] = 0.
    init_solution = pyclaw.Solution(state)
    solver.mwaves = 2
    solver.limiters = [4] * solver.mwaves
    solver.dt_initial = grid.d[0] / state.aux_global['cc'] * 0.1
    solver.bc_lower[0] = pyclaw.BC.periodic
    solver.bc_upper[0] = pyclaw.BC.periodic
    claw = pyclaw.Controller()
    claw.keep_copy = True
    claw.nout = 5
    claw.tfinal = 1.0
    claw.solution = init_solution
    claw.solver = solver
    if not run:
        return None, claw
    claw.run()
    q0 = claw.frames[0].state.q.reshape([-1])
    qfinal = claw.frames[claw.nout].state.q.reshape([-1])
    dx = claw.frames[0].grid.d[0]
    return dx * np.sum(np.abs(qfinal - q0)), claw


def advection1D(pyclaw, mx=1000, tfinal=1.0, nout=10):
    """apps/advection/1d/constant/advection.py:3-44 at the C1 size (1000 cells)."""
    solver = pyclaw.ClawSolver1D()
    solver.rp = pyclaw.riemann.rp_advection_1d
    solver.mwaves = 1
    solver.bc_lower[0] = 2
    solver.bc_upper[0] = 2
    x = pyclaw.Dimension('x', 0.0, 1.0, mx)
    grid = pyclaw.Grid(x)
    state = pyclaw.State(grid, 1)
    state.aux_global['u'] = 1.
    xc = grid.x.center
    beta = 100
    gam = 0
    x0 = 0.75
    state.q[0, :] = np.exp(-beta * (xc - x0) ** 2) * np.cos(gam * (xc - x0))
    claw = pyclaw.Controller()
    claw.keep_copy = True
    claw.solution = pyclaw.Solution(state)
    claw.solver = solver
    claw.tfinal = tfinal
    claw.nout = nout
    claw.run()
    return claw


def acoustics3D(pyclaw, test='hom', mx=None, my=None, mz=None, run=True, math='exact', tfinal=2.0, nout=10, user_rp=False,
                solver_type='classic', lim_type=2, weno_order=5, time_integrator='SSP104'):
    """test/acoustics/3d/acoustics.py:6-96.  'hom': dim-split 256x4x4, all periodic (the reference gates
    final_difference = 0.00286 +- 1e-4, test/test_examples.py:481-488); 'het' needs the unsplit step3.  user_rp=True:
    the same solver as the body VC_ACOUSTICS_3D_RP of a pyclaw.CellRiemann3D, for 'het' with the transverse bodies
    VC_ACOUSTICS_3D_RPT / VC_ACOUSTICS_3D_RPTT.  solver_type='sharpclaw': SharpClawSolver3D with the same body in a
    pyclaw.SharpCellRiemann3D (SharpClaw in 3-D runs solvers compiled at run time only), either test's set-up."""
    sharp = solver_type == 'sharpclaw'
    solver = pyclaw.SharpClawSolver3D() if sharp else pyclaw.ClawSolver3D()
    solver.math = math
    trans = {} if test == 'hom' else dict(rpt3=VC_ACOUSTICS_3D_RPT, rptt3=VC_ACOUSTICS_3D_RPTT)
    if sharp:
        solver.rp = pyclaw.SharpCellRiemann3D(VC_ACOUSTICS_3D_RP, 4, 2, aux=(0, 1), name="vc_acoustics_3d_sharp")
        solver.lim_type, solver.weno_order, solver.time_integrator = lim_type, weno_order, time_integrator
    else:
        solver.rp = (pyclaw.CellRiemann3D(VC_ACOUSTICS_3D_RP, 4, 2, aux=(0, 1), name="vc_acoustics_3d_user", **trans) if user_rp
                     else pyclaw.riemann.rp_vc_acoustics_3d)
    for k in range(3):
        solver.bc_lower[k] = solver.bc_upper[k] = pyclaw.BC.periodic
        solver.aux_bc_lower[k] = solver.aux_bc_upper[k] = pyclaw.BC.periodic
    if test == 'hom':
        if not sharp:
            solver.dim_split = True
        mx, my, mz = mx or 256, my or 4, mz or 4
        zr = cr = 1.0
    else:
        if not sharp:
            solver.dim_split = False
        for k in range(3):
            solver.bc_lower[k] = pyclaw.BC.reflecting
            solver.aux_bc_lower[k] = pyclaw.BC.reflecting
        mx, my, mz = mx or 30, my or 30, mz or 30
        zr = cr = 2.0
    solver.mwaves = 2
    solver.limiters = pyclaw.limiters.tvd.MC
    x = pyclaw.Dimension('x', -1.0, 1.0, mx)
    y = pyclaw.Dimension('y', -1.0, 1.0, my)
    z = pyclaw.Dimension('z', -1.0, 1.0, mz)
    grid = pyclaw.Grid([x, y, z])
    state = pyclaw.State(grid, 4, 2)
    zl = cl = 1.0
    grid.compute_c_center()
    X, Y, Z = grid._c_center
    state.aux[0, :, :, :] = zl * (X < 0.) + zr * (X >= 0.)
    state.aux[1, :, :, :] = cl * (X < 0.) + cr * (X >= 0.)
    x0, y0, z0 = -0.5, 0., 0.
    if test == 'hom':
        r = np.sqrt((X - x0) ** 2)
        width = 0.2
        state.q[0, :, :, :] = (np.abs(r) <= width) * (1. + np.cos(np.pi * r / width))
    else:
        r = np.sqrt((X - x0) ** 2 + (Y - y0) ** 2 + (Z - z0) ** 2)
        width = 0.1
        state.q[0, :, :, :] = (np.abs(r - 0.3) <= width) * (1. + np.cos(np.pi * (r - 0.3) / width))
    state.q[1:, :, :, :] = 0.
    claw = pyclaw.Controller()
    claw.keep_copy = True
    claw.solution = pyclaw.Solution(state)
    claw.solver = solver
    claw.tfinal = tfinal
    claw.nout = nout
    if not run:
        return claw
    claw.run()
    return claw


def euler3D(pyclaw, axis=0, n=64, across=(4, 4), tfinal=0.1, nout=1, run=True, math='exact', order=2, dim_split=True,
            order_trans=22, solver_type='classic', lim_type=2, weno_order=5, time_integrator='SSP104'):
    """A system the library has no 3-D solver for: the Euler equations through EULER_3D_RP in a pyclaw.CellRiemann3D.
    Sod's jump across the plane through the middle of the box normal to `axis` (0, 1, 2), n cells along that axis and
    `across` cells along the other two (in cyclic order), extrapolation on every side; the dimension-split step or,
    dim_split=False, the unsplit one with the transverse bodies EULER_3D_RPT / EULER_3D_RPTT and `order_trans`.
    solver_type='sharpclaw': SharpClawSolver3D with the body in a pyclaw.SharpCellRiemann3D."""
    sharp = solver_type == 'sharpclaw'
    solver = pyclaw.SharpClawSolver3D() if sharp else pyclaw.ClawSolver3D()
    solver.math = math
    if sharp:
        solver.rp = pyclaw.SharpCellRiemann3D(EULER_3D_RP, 5, 3, params=[gamma], name="euler_3d_sharp")
        solver.lim_type, solver.weno_order, solver.time_integrator = lim_type, weno_order, time_integrator
    else:
        trans = {} if dim_split else dict(rpt3=EULER_3D_RPT, rptt3=EULER_3D_RPTT)
        solver.rp = pyclaw.CellRiemann3D(EULER_3D_RP, 5, 3, params=[gamma], name="euler_3d_user", **trans)
        solver.dim_split = bool(dim_split)
        if not dim_split:
            solver.order_trans = order_trans
        solver.order = order
        solver.limiters = [4, 4, 4]
    solver.mwaves = 3
    for k in range(3):
        solver.bc_lower[k] = solver.bc_upper[k] = pyclaw.BC.outflow
    cells = [0, 0, 0]
    cells[axis], cells[(axis + 1) % 3], cells[(axis + 2) % 3] = n, across[0], across[1]
    # (unit cells in all three directions: a permutation of the axes is a permutation of the problem)
    d = 1.0 / n
    dims = [pyclaw.Dimension(name, 0.0, cells[k] * d, cells[k]) for k, name in enumerate('xyz')]
    grid = pyclaw.Grid(dims)
    state = pyclaw.State(grid, 5)
    grid.compute_c_center()
    along = grid._c_center[axis]
    left = along < 0.5
    state.q[0] = np.where(left, 1.0, 0.125)
    state.q[1:4] = 0.0
    state.q[4] = np.where(left, 1.0, 0.1) / gamma1
    claw = pyclaw.Controller()
    claw.keep_copy = True
    claw.solution = pyclaw.Solution(state)
    claw.solver = solver
    claw.tfinal, claw.nout = tfinal, nout
    solver.dt_initial = 0.2 * d
    if not run:
        return claw
    claw.run()
    return claw


# ---------------------------------------------------------------------------------------------------
# Further set-ups in the style of the reference's apps/ directory (no golden in the reference: the GPU tests check
# them against exact physics or the oracle driver, tests/test_gpu_more_solvers.py)
# ---------------------------------------------------------------------------------------------------
def sod_shock_tube(pyclaw, n=800, tfinal=0.2, solver_type='classic'):
    """apps/euler/1d style: Sod's Riemann problem with rp_euler_1d (Roe + entropy fix)."""
    solver = pyclaw.ClawSolver1D() if solver_type == 'classic' else pyclaw.SharpClawSolver1D()
    solver.rp = pyclaw.riemann.rp_euler_1d
    solver.mwaves = 3
    solver.limiters = [4, 4, 4]
    solver.bc_lower[0] = solver.bc_upper[0] = pyclaw.BC.outflow
    state = pyclaw.State(pyclaw.Grid(pyclaw.Dimension('x', 0.0, 1.0, n)), 3)
    state.aux_global['gamma'] = gamma
    state.aux_global['gamma1'] = gamma1
    xc = state.grid.x.center
    state.q[0] = np.where(xc < 0.5, 1.0, 0.125)
    state.q[1] = 0.0
    state.q[2] = np.where(xc < 0.5, 1.0, 0.1) / gamma1
    claw = pyclaw.Controller()
    claw.keep_copy = True
    claw.solution = pyclaw.Solution(state)
    claw.solver = solver
    claw.tfinal, claw.nout = tfinal, 1
    solver.dt_initial = 1e-4
    claw.run()
    return claw


def radial_dam_break(pyclaw, n=200, tfinal=1.0, dim_split=False, solver_type='classic'):
    """apps/shallow/2d style: radial dam break with rp_shallow_2d (Roe + entropy fix, transverse solver)."""
    solver = pyclaw.ClawSolver2D() if solver_type == 'classic' else pyclaw.SharpClawSolver2D()
    solver.rp = pyclaw.riemann.rp_shallow_2d
    solver.mwaves = 3
    solver.limiters = [4, 4, 4]
    if solver_type == 'classic':
        solver.dim_split = dim_split
        solver.order_trans = 2
    for k in range(2):
        solver.bc_lower[k] = solver.bc_upper[k] = pyclaw.BC.outflow
    grid = pyclaw.Grid([pyclaw.Dimension('x', -2.5, 2.5, n), pyclaw.Dimension('y', -2.5, 2.5, n)])
    state = pyclaw.State(grid, 3)
    state.aux_global['g'] = 1.0
    X, Y = grid.c_center
    r = np.sqrt(X ** 2 + Y ** 2)
    state.q[0] = 2.0 * (r <= 0.5) + 1.0 * (r > 0.5)
    state.q[1:] = 0.0
    claw = pyclaw.Controller()
    claw.keep_copy = True
    claw.solution = pyclaw.Solution(state)
    claw.solver = solver
    claw.tfinal, claw.nout = tfinal, 1
    solver.dt_initial = 1e-3
    claw.run()
    return claw


def burgers_1d(pyclaw, n=400, tfinal=0.5):
    """apps/burgers/1d style: a step that steepens into a shock moving at the Rankine-Hugoniot speed 1/2."""
    solver = pyclaw.ClawSolver1D()
    solver.rp = pyclaw.riemann.rp_burgers_1d
    solver.mwaves = 1
    solver.limiters = pyclaw.limiters.tvd.vanleer
    solver.bc_lower[0] = solver.bc_upper[0] = pyclaw.BC.outflow
    state = pyclaw.State(pyclaw.Grid(pyclaw.Dimension('x', 0.0, 1.0, n)), 1)
    state.q[0, :] = 1.0 * (state.grid.x.center < 0.25)
    claw = pyclaw.Controller()
    claw.keep_copy = True
    claw.solution = pyclaw.Solution(state)
    claw.solver = solver
    claw.tfinal, claw.nout = tfinal, 1
    solver.dt_initial = 0.001
    claw.run()
    return claw


def rotating_flow(pyclaw, n=64, solver_type='classic', tfinal=0.3, run=True):
    """Solid-body-like rotation of a blob: colour equation (rp_vc_advection_2d) with edge velocities from a stream
    function and a capacity function in aux(3) -- the ingredients of apps/advection/2d/annulus on a Cartesian grid --
    periodic in both directions; classic unsplit (order_trans 2, van Leer) or SharpClaw WENO5."""
    if solver_type == "classic":
        solver = pyclaw.ClawSolver2D()
        solver.dim_split = False
        solver.order_trans = 2
        solver.limiters = pyclaw.limiters.tvd.vanleer
        solver.cfl_max, solver.cfl_desired = 1.0, 0.9
    else:
        solver = pyclaw.SharpClawSolver2D()
        solver.lim_type = 2
    solver.rp = pyclaw.riemann.rp_vc_advection_2d
    solver.mwaves = 1
    for k in range(2):
        solver.bc_lower[k] = solver.bc_upper[k] = pyclaw.BC.periodic
        solver.aux_bc_lower[k] = solver.aux_bc_upper[k] = pyclaw.BC.periodic
    grid = pyclaw.Grid([pyclaw.Dimension('x', -1.0, 1.0, n), pyclaw.Dimension('y', -1.0, 1.0, n)])
    state = pyclaw.State(grid, 1, 3)
    state.mcapa = 2
    d = grid.d[0]
    xe, ye = grid.x.edge, grid.y.edge
    psi = lambda x, y: 0.5 * np.pi * (np.cos(np.pi * x / 2) ** 2) * (np.cos(np.pi * y / 2) ** 2)   # stream function
    XE, YE = np.meshgrid(xe, ye, indexing="ij")
    P = psi(XE, YE)
    state.aux[0] = (P[:-1, 1:] - P[:-1, :-1]) / d          # u at the left edge   =  d(psi)/dy
    state.aux[1] = -(P[1:, :-1] - P[:-1, :-1]) / d         # v at the bottom edge = -d(psi)/dx
    X, Y = grid.c_center
    state.aux[2] = 1.0 + 0.2 * np.sin(np.pi * X) * np.sin(np.pi * Y)    # capacity
    state.q[0] = np.exp(-40.0 * ((X - 0.3) ** 2 + Y ** 2))
    claw = pyclaw.Controller()
    claw.keep_copy = True
    claw.solution = pyclaw.Solution(state)
    claw.solver = solver
    claw.tfinal, claw.nout = tfinal, 1
    solver.dt_initial = 0.005
    if run:
        claw.run()
    return claw


# ---------------------------------------------------------------------------------------------------
# Cell functions that read neighbour cells (reach > 0: qn / auxn), each with its numpy twin.  A twin forms the right-hand
# side from a padded copy of the OLD interior and then assigns, in the body's operation order, so that the 'exact'
# arithmetic gives the same bits.
# ---------------------------------------------------------------------------------------------------
def pad_like_bcs(a, reach, modes, normal0=1):
    """The interior array a[m, ...] with `reach` ghost layers, filled like apply_q_bcs: per dimension (x first, so the
    corners match), lower then upper, each side by np.pad in the mode that equals its boundary condition --
    'wrap' (periodic), 'edge' (zero-order extrapolation), 'wall' (mirrored, the normal component normal0 + idim negated),
    or a sequence of one constant per component (a constant inflow state).  modes[idim] = (lower, upper) or one mode."""
    for idim in range(a.ndim - 1):
        mode = modes[idim]
        lower, upper = (mode, mode) if isinstance(mode, str) else mode
        axis = idim + 1
        strips = []
        for side, md in ((0, lower), (1, upper)):
            width = [(0, 0)] * a.ndim
            width[axis] = (reach, 0) if side == 0 else (0, reach)
            take = [slice(None)] * a.ndim
            take[axis] = slice(0, reach) if side == 0 else slice(a.shape[axis], None)
            if isinstance(md, str):
                g = np.pad(a, width, mode={'wrap': 'wrap', 'edge': 'edge', 'wall': 'symmetric'}[md])[tuple(take)].copy()
                if md == 'wall':
                    g[normal0 + idim] = -g[normal0 + idim]
            else:
                g = np.stack([np.pad(a[m], width[1:], mode='constant', constant_values=float(v))[tuple(take[1:])]
                              for m, v in enumerate(md)])
            strips.append(g)
        a = np.concatenate([strips[0], a, strips[1]], axis=axis)
    return a


def shifted(qb, reach, off):
    """the interior-sized window of the padded array qb at index offset off[idim]"""
    return qb[(slice(None),) + tuple(slice(reach + o, qb.shape[k + 1] - reach + o) for k, o in enumerate(off))]


# q_t = nu * Laplace(q), forward Euler over c.dt, second-order differences: 5 points in 2-D, 7 in 3-D.  p[0] = nu,
# p[1] = the number of leading components it acts on (0: all of them)
DIFFUSION_2D_CELL_SRC = """
const int nm = p[1] > 0.0 ? (int)p[1] : MEQN;
for (int m = 0; m < MEQN; m++) {
    if (m >= nm) break;
    const double lx = (qn(m, 1, 0) - 2.0 * qn(m, 0, 0) + qn(m, -1, 0)) / (c.d[0] * c.d[0]);
    const double ly = (qn(m, 0, 1) - 2.0 * qn(m, 0, 0) + qn(m, 0, -1)) / (c.d[1] * c.d[1]);
    q[m] = q[m] + c.dt * p[0] * (lx + ly);
}
"""

DIFFUSION_3D_CELL_SRC = """
const int nm = p[1] > 0.0 ? (int)p[1] : MEQN;
for (int m = 0; m < MEQN; m++) {
    if (m >= nm) break;
    const double lx = (qn(m, 1, 0, 0) - 2.0 * qn(m, 0, 0, 0) + qn(m, -1, 0, 0)) / (c.d[0] * c.d[0]);
    const double ly = (qn(m, 0, 1, 0) - 2.0 * qn(m, 0, 0, 0) + qn(m, 0, -1, 0)) / (c.d[1] * c.d[1]);
    const double lz = (qn(m, 0, 0, 1) - 2.0 * qn(m, 0, 0, 0) + qn(m, 0, 0, -1)) / (c.d[2] * c.d[2]);
    q[m] = q[m] + c.dt * p[0] * (lx + ly + lz);
}
"""


def diffusion_src(nu, modes, ncomp=0, calls=None):
    """numpy twin of DIFFUSION_2D_CELL_SRC / DIFFUSION_3D_CELL_SRC as a step_src(solver, state, dt); modes as for
    pad_like_bcs.  calls: a list that gets one entry per call."""
    def step_src(solver, state, dt):
        if calls is not None:
            calls.append(dt)
        q = state.q
        nd = q.ndim - 1
        nm = ncomp if ncomp > 0 else q.shape[0]
        qb = pad_like_bcs(q, 1, modes)
        zero = (0,) * nd
        lap = 0.0
        for k in range(nd):
            up, dn = tuple(int(j == k) for j in range(nd)), tuple(-int(j == k) for j in range(nd))
            lk = (shifted(qb, 1, up) - 2.0 * shifted(qb, 1, zero) + shifted(qb, 1, dn)) / (state.grid.d[k] * state.grid.d[k])
            lap = lk if k == 0 else lap + lk
        q[:nm] = (q + dt * nu * lap)[:nm]
    return step_src


# SharpClaw dq_src: dt * nu * (4th-order Laplacian), reach = 2, 1-D and 2-D.  p[0] = nu
LAPLACIAN4_DQ_CELL_SRC = """
for (int m = 0; m < MEQN; m++) {
    double lap = (-qn(m, -2) + 16.0 * qn(m, -1) - 30.0 * qn(m, 0) + 16.0 * qn(m, 1) - qn(m, 2)) / (12.0 * c.d[0] * c.d[0]);
#if NDIM > 1
    lap = lap + (-qn(m, 0, -2) + 16.0 * qn(m, 0, -1) - 30.0 * qn(m, 0, 0) + 16.0 * qn(m, 0, 1) - qn(m, 0, 2))
                / (12.0 * c.d[1] * c.d[1]);
#endif
    dq[m] = c.dt * p[0] * lap;
}
"""


def laplacian4_dq_src(nu, modes):
    """numpy twin of LAPLACIAN4_DQ_CELL_SRC as a dq_src(solver, state, dt)"""
    def dq_src(solver, state, dt):
        q = state.q
        nd = q.ndim - 1
        qb = pad_like_bcs(q, 2, modes)
        lap = 0.0
        for k in range(nd):
            at = lambda o: shifted(qb, 2, tuple(o * int(j == k) for j in range(nd)))
            d = state.grid.d[k]
            lk = (-at(-2) + 16.0 * at(-1) - 30.0 * at(0) + 16.0 * at(1) - at(2)) / (12.0 * d * d)
            lap = lk if k == 0 else lap + lk
        return dt * nu * lap
    return dq_src


# a force from the x gradient of a potential kept in aux(1), central difference: p[0] = its strength
AUX_GRADIENT_CELL_SRC = """
q[1] -= c.dt * p[0] * (auxn(0, 1, 0) - auxn(0, -1, 0)) / (2.0 * c.d[0]);
"""


def aux_gradient_src(g):
    """numpy twin of AUX_GRADIENT_CELL_SRC, on the solver's ghosted aux (solver.auxbc)"""
    def step_src(solver, state, dt):
        mbc = solver.mbc
        a = solver.auxbc[0][:, mbc:-mbc]
        n = state.q.shape[1]
        state.q[1] -= dt * g * (a[mbc + 1:mbc + 1 + n] - a[mbc - 1:mbc - 1 + n]) / (2.0 * state.grid.d[0])
    return step_src


# the four diagonal neighbours' mean: what shows the corner ghost cells
DIAGONAL_MEAN_CELL_HOOK = "q[0] = 0.25 * (qn(0, 1, 1) + qn(0, -1, 1) + qn(0, 1, -1) + qn(0, -1, -1));"


def diagonal_mean_hook(modes):
    """numpy twin of DIAGONAL_MEAN_CELL_HOOK as a start_step(solver, solution)"""
    def start_step(solver, solution):
        q = solution.state.q
        qb = pad_like_bcs(q, 1, modes)
        q[0] = (0.25 * (shifted(qb, 1, (1, 1)) + shifted(qb, 1, (-1, 1)) + shifted(qb, 1, (1, -1)) + shifted(qb, 1, (-1, -1))))[0]
    return start_step


def advection2D(pyclaw, mx=37, my=21, bc_y=None):
    """A blob carried by the constant velocity (0.5, 1) on the unit square, periodic in x and (unless bc_y is given) in
    y, dimension-split: (solver, solution), not set up."""
    solver = pyclaw.ClawSolver2D()
    solver.rp = pyclaw.riemann.rp_advection_2d
    solver.mwaves = 1
    solver.dim_split = True
    solver.limiters = pyclaw.limiters.tvd.MC
    solver.bc_lower[0] = solver.bc_upper[0] = pyclaw.BC.periodic
    solver.bc_lower[1] = solver.bc_upper[1] = pyclaw.BC.periodic if bc_y is None else bc_y
    grid = pyclaw.Grid([pyclaw.Dimension('x', 0.0, 1.0, mx), pyclaw.Dimension('y', 0.0, 1.0, my)])
    state = pyclaw.State(grid, 1)
    state.aux_global['u'] = 0.5
    state.aux_global['v'] = 1.0
    X, Y = grid.c_center
    state.q[0] = np.exp(-30.0 * ((X - 0.3) ** 2 + (Y - 0.6) ** 2)) + 0.1 * X + 0.05 * Y * Y
    return solver, pyclaw.Solution(state)


def fixed_steps(solver, solution, nsteps, dt):
    """setup(), nsteps steps of length dt, teardown(): the final q"""
    solver.dt_variable = False
    solver.setup(solution)
    solver.dt = dt
    for n in range(nsteps):
        solver.evolve_to_time(solution)
    solver.teardown()
    return solution.state.q.copy('F')
