"""Stand-in for the PyPI package `airfoils` (absent from this image, no network).

TEST INFRASTRUCTURE ONLY -- used by oracle/gen_golden.py so that the *unmodified* reference class
(/root/reference/LUDVM.py) can run end-to-end here.  The reference touches the package only at
LUDVM.py:301-302, 312, 328-335, and for a symmetric NACA 00xx section everything it takes from it
reduces to a camber line that is identically zero (eta == 0 at LUDVM.py:335,340), independent of
the package's point distribution.  By default anything else (cambered digits) raises, so no golden
vector can silently depend on arithmetic this stand-in does not reproduce.

The one opt-in: MEAN_LINE.  oracle/gen_golden.py sets it for fixture group G10 alone (and puts None
back), to a function (digits, x) -> camber / chord -- oracle/ludvm_oracle.py::naca4_camber, the
published NACA 4-digit mean line.  `camber_line(x)` then returns that function's value at the
stand-in's own stations linspace(0, 1, n_points).
  What this pins: everything the reference does DOWNSTREAM of the mean line -- its interpolation onto
  the theta-uniform nodes and the panel quarter points, the slopes, the camber terms of downwash and
  solve, the bound-vortex positions, the loads and the flow field.
  What it does not pin: the mean line itself as the PyPI package would hand it over -- that package's
  point distribution and its formula -- and sections read from .dat files (airfoils.fileio and a cubic
  interpolant).
"""
import numpy as np

MEAN_LINE = None        # None: symmetric sections only.  Set by oracle/gen_golden.py for G10 and by nothing else.


class Airfoil:
    def __init__(self, n_points, digits="0012"):
        xs = np.linspace(0.0, 1.0, n_points)
        self._digits = digits
        self._x_upper = xs
        self._x_lower = xs.copy()
        self._y_upper = np.zeros(n_points)   # thickness is never read by the reference
        self._y_lower = np.zeros(n_points)
        self.all_points = np.zeros((2, 2 * n_points))

    @classmethod
    def NACA4(cls, naca_digits, n_points=200):
        if len(naca_digits) != 4:
            raise NotImplementedError("airfoils stand-in only covers NACA 4-digit sections")
        if naca_digits[:2] != "00" and MEAN_LINE is None:
            raise NotImplementedError("airfoils stand-in only covers symmetric NACA 00xx sections (cambered digits: MEAN_LINE)")
        return cls(n_points, naca_digits)

    def camber_line(self, x):
        x = np.asarray(x, dtype=float)
        if self._digits[:2] == "00" or MEAN_LINE is None:
            return np.zeros_like(x)
        return MEAN_LINE(self._digits, x)

    def camber_line_angle(self, x):
        return np.zeros_like(np.asarray(x, dtype=float))   # (LUDVM.py:333 stores it and never reads it)
