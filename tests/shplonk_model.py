"""Integer model of the Shplonk openings (include/kzg_gpu.h, "Shplonk openings"), shared by
tests/test_shplonk_abi.py and tests/test_gpu_shplonk.py.  Python integers mod r only: nothing here
touches the library.  With a known tau every commitment and proof is a known multiple of G, so the
verifier's pairing equation is an equation on exponents."""


def ev(r, P, x):
    acc = 0
    for a in reversed(P):
        acc = (acc * x + a) % r
    return acc


def poly_mul_linear(r, Z, t):
    """Z (X - t)"""
    out = [0] * (len(Z) + 1)
    for i, a in enumerate(Z):
        out[i + 1] = (out[i + 1] + a) % r
        out[i] = (out[i] - a * t) % r
    return out


def floor_div(r, F, Z):
    """schoolbook F div Z for monic Z; len(F) - len(Z) + 1 coefficients ([] when deg F < deg Z)"""
    F = list(F)
    d = len(Z) - 1
    assert Z[-1] == 1
    if len(F) <= d:
        return []
    q = [0] * (len(F) - d)
    for i in range(len(F) - 1, d - 1, -1):
        c = F[i]
        q[i - d] = c
        if c:
            for j, z in enumerate(Z):
                F[i - d + j] = (F[i - d + j] - c * z) % r
    return q


def single_quotient(r, F, t):
    """(F - F(t)) / (X - t): len(F) - 1 coefficients"""
    q = [0] * (len(F) - 1)
    acc = 0
    for k in range(len(F) - 1, 0, -1):
        acc = (F[k] + acc * t) % r
        q[k - 1] = acc
    return q


class Table:
    """polys: lists of n coefficients; T: the points; sets: (point indices, claim indices) pairs, the claim
    indices naming polynomials (= commitments); w: one weight per claim, set by set"""

    def __init__(self, r, polys, T, sets, w):
        self.r, self.polys, self.T, self.sets, self.w = r, polys, list(T), [(list(a), list(b)) for a, b in sets], list(w)
        self.n = len(polys[0]) if polys else 0
        self.index = [j for _, cl in self.sets for j in cl]
        self.claim_start = [0]
        self.set_point_start = [0]
        for pts, cl in self.sets:
            self.claim_start.append(self.claim_start[-1] + len(cl))
            self.set_point_start.append(self.set_point_start[-1] + len(pts))
        self.set_points = [i for pts, _ in self.sets for i in pts]
        assert len(self.w) == len(self.index)
        self.n_values = sum(len(a) * len(b) for a, b in self.sets)

    def claims(self, s):
        return range(self.claim_start[s], self.claim_start[s + 1])

    def folded(self, s):
        r = self.r
        return [sum(self.w[k] * self.polys[self.index[k]][i] for k in self.claims(s)) % r for i in range(self.n)]

    def vanishing(self, s):
        Z = [1]
        for i in self.sets[s][0]:
            Z = poly_mul_linear(self.r, Z, self.T[i])
        return Z

    def h(self):
        """sum_s F_s div Z_s by schoolbook division, n coefficients (h[n-1] = 0)"""
        r = self.r
        out = [0] * self.n
        for s in range(len(self.sets)):
            for i, a in enumerate(floor_div(r, self.folded(s), self.vanishing(s))):
                out[i] = (out[i] + a) % r
        return out

    def values(self):
        """claim by claim, each claim's d_s values in the set's point order"""
        return [ev(self.r, self.polys[j], self.T[i]) for pts, cl in self.sets for j in cl for i in pts]

    def zeta(self, s, z):
        r, inside = self.r, set(self.sets[s][0])
        out = 1
        for i, t in enumerate(self.T):
            if i not in inside:
                out = out * (z - t) % r
        return out

    def z_T(self, z):
        out = 1
        for t in self.T:
            out = out * (z - t) % self.r
        return out

    def lagrange_at(self, s, z):
        """l_(s,i)(z) for the set's points, in product form; ZeroDivisionError/ValueError on equal values"""
        r, pts = self.r, self.sets[s][0]
        out = []
        for a in pts:
            num = den = 1
            for b in pts:
                if b != a:
                    num = num * (z - self.T[b]) % r
                    den = den * (self.T[a] - self.T[b]) % r
            out.append(num * pow(den, -1, r) % r)
        return out

    def G(self, h, z):
        r = self.r
        zt = self.z_T(z)
        out = [(-zt * a) % r for a in h]
        for s in range(len(self.sets)):
            zs = self.zeta(s, z)
            for k in self.claims(s):
                c = zs * self.w[k] % r
                P = self.polys[self.index[k]]
                for i in range(self.n):
                    out[i] = (out[i] + c * P[i]) % r
        return out

    def verifier_scalars(self, ys, z, n_commits):
        """s_c and t"""
        r = self.r
        s_c = [0] * n_commits
        t = 0
        v = 0
        for s, (pts, cl) in enumerate(self.sets):
            zs = self.zeta(s, z)
            L = self.lagrange_at(s, z)
            for kk, j in enumerate(cl):
                k = self.claim_start[s] + kk
                rk = sum(ys[v + i] * L[i] for i in range(len(pts))) % r
                v += len(pts)
                s_c[j] = (s_c[j] + zs * self.w[k]) % r
                t = (t + zs * self.w[k] * rk) % r
        return s_c, t

    def verify(self, tau, commits, ys, z, W, Wp):
        """the header's equation on exponents: commits, W, Wp are multiples of G"""
        r = self.r
        s_c, t = self.verifier_scalars(ys, z, len(commits))
        rhs = (sum(a * b for a, b in zip(s_c, commits)) - t - self.z_T(z) * W + z * Wp) % r
        return (tau * Wp - rhs) % r == 0


def powers(r, gamma, count):
    return [pow(gamma, k, r) for k in range(count)]
