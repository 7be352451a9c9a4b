// Dense / sparse helpers of the statistical models that consume the PDE solver, written on the
// facade's own containers so that they compile where Eigen is absent:
//   lump(A)              row-sum lumping                    fdaPDE/linear_algebra/lumping.h:30-51
//   PartialPivLU         small dense LU (q x q)             stands in for Eigen::PartialPivLU<DMatrix<double>>
//   SMW<SparseSolver>    Sherman-Morrison-Woodbury solve    fdaPDE/linear_algebra/smw.h:38-59
//   SparseBlockMatrix<double,2,2>   four sparse blocks as one matrix   fdaPDE/linear_algebra/sparse_block_matrix.h:29-128
//                        (what PDE::BlockSolver factors: SMW<PDE<...>::BlockSolver> solves the smoothing system under a low-rank update; the data term
//                        Psi^T W Psi may stay factored -- BlockSolver::compute(A, Psi, weights, scale), set_observations -- which is the only door for an
//                        areal Psi, whose Psi^T Psi does not lie on the pattern a block must lie on)
//   Kronecker(T, S), KroneckerSum   lazy dense (x) sparse products and their sums   fdaPDE/linear_algebra/kronecker_product.h:56-80
//                        (what PDE::KroneckerSolver factors without forming the product: the space-time systems; eval() gives the explicit matrix)
//                        (the data term (Phi (x) Psi)^T W (Phi (x) Psi) may stay factored -- KroneckerSolver::compute(A, Phi, Psi, weights, scale),
//                        set_observations --: areal designs, missing observations and observation instants off the time nodes)
// The heavy step of SMW, A^{-1} [b | U] (1 + q right-hand sides against one prepared sparse system), runs on the device as ONE
// batched multi-column solve through the factor-once handle (PDE::SparseSolver -> fdapde_lin_compute / fdapde_lin_solve);
// everything dense is q x q or n x q host work.
#ifndef FDAPDE_AMD_LINEAR_ALGEBRA_H
#define FDAPDE_AMD_LINEAR_ALGEBRA_H

#include <algorithm>
#include <array>
#include <cmath>
#include <stdexcept>
#include <utility>
#include <vector>

#include "pde.h"

namespace fdapde {
namespace amd {

// ---- dense products / sums on column-major DMatrix ---------------------------------------------------------------------
inline DMatrix<double> operator*(const DMatrix<double>& a, const DMatrix<double>& b) {
    if (a.cols() != b.rows()) throw std::runtime_error("DMatrix product: inner dimensions differ");
    DMatrix<double> c(a.rows(), b.cols(), 0.0);
    for (int64_t j = 0; j < b.cols(); ++j)
        for (int64_t k = 0; k < a.cols(); ++k) {
            const double bkj = b(k, j);
            for (int64_t i = 0; i < a.rows(); ++i) c(i, j) += a(i, k) * bkj;
        }
    return c;
}
inline DMatrix<double> operator+(const DMatrix<double>& a, const DMatrix<double>& b) {
    if (a.rows() != b.rows() || a.cols() != b.cols()) throw std::runtime_error("DMatrix sum: shapes differ");
    DMatrix<double> c(a.rows(), a.cols());
    for (int64_t i = 0; i < a.size(); ++i) c.data()[i] = a.data()[i] + b.data()[i];
    return c;
}
inline DMatrix<double> operator-(const DMatrix<double>& a, const DMatrix<double>& b) {
    if (a.rows() != b.rows() || a.cols() != b.cols()) throw std::runtime_error("DMatrix difference: shapes differ");
    DMatrix<double> c(a.rows(), a.cols());
    for (int64_t i = 0; i < a.size(); ++i) c.data()[i] = a.data()[i] - b.data()[i];
    return c;
}
inline DMatrix<double> transpose(const DMatrix<double>& a) {
    DMatrix<double> t(a.cols(), a.rows());
    for (int64_t j = 0; j < a.cols(); ++j)
        for (int64_t i = 0; i < a.rows(); ++i) t(j, i) = a(i, j);
    return t;
}

// ---- lumping (lumping.h:30-41): diagonal sparse matrix of the row sums -------------------------------------------------
template <typename T> SpMatrix<T> lump(const SpMatrix<T>& a) {
    if (a.rows() != a.cols()) throw std::runtime_error("lump: matrix must be square");   // fdapde_assert, lumping.h:31
    SpMatrix<T> d;
    d.n_rows = d.n_cols = a.rows();
    d.rowptr.resize((size_t)a.rows() + 1);
    d.colidx.resize((size_t)a.rows());
    d.values.resize((size_t)a.rows());
    for (int64_t i = 0; i < a.rows(); ++i) {
        T s = 0;
        for (int32_t k = a.rowptr[(size_t)i]; k < a.rowptr[(size_t)i + 1]; ++k) s += a.values[(size_t)k];
        d.rowptr[(size_t)i] = (int32_t)i, d.colidx[(size_t)i] = (int32_t)i, d.values[(size_t)i] = s;
    }
    d.rowptr[(size_t)a.rows()] = (int32_t)a.rows();
    return d;
}

// ---- SparseBlockMatrix<T, 2, 2> (sparse_block_matrix.h:29-128): the blocks in row-major order, as the reference's constructor takes them ----------
template <typename T, int Rows, int Cols> class SparseBlockMatrix;
template <typename T> class SparseBlockMatrix<T, 2, 2> {
   public:
    SparseBlockMatrix() = default;
    SparseBlockMatrix(const SpMatrix<T>& m00, const SpMatrix<T>& m01, const SpMatrix<T>& m10, const SpMatrix<T>& m11) : blocks_ {m00, m01, m10, m11} {
        // blocks of a block row share their rows, blocks of a block column their columns (sparse_block_matrix.h:60-72)
        if (m00.rows() != m01.rows() || m10.rows() != m11.rows() || m00.cols() != m10.cols() || m01.cols() != m11.cols())
            throw std::runtime_error("SparseBlockMatrix: the blocks do not fit together");
        rows_ = m00.rows() + m10.rows(), cols_ = m00.cols() + m01.cols();
    }
    const SpMatrix<T>& block(int i, int j) const { return blocks_[(size_t)(2 * i + j)]; }
    int64_t rows() const { return rows_; }
    int64_t cols() const { return cols_; }
    int64_t nonZeros() const {
        int64_t s = 0;
        for (const auto& b : blocks_) s += b.nonZeros();
        return s;
    }
    T coeff(int64_t i, int64_t j) const {
        const int64_t r0 = blocks_[0].rows(), c0 = blocks_[0].cols();
        return block(i >= r0, j >= c0).coeff(i >= r0 ? i - r0 : i, j >= c0 ? j - c0 : j);
    }
    DMatrix<T> operator*(const DMatrix<T>& x) const {   // host-side product (checks)
        const int64_t r0 = blocks_[0].rows(), c0 = blocks_[0].cols();
        DMatrix<T> y(rows_, x.cols(), T(0));
        for (int bi = 0; bi < 2; ++bi)
            for (int bj = 0; bj < 2; ++bj) {
                const SpMatrix<T>& b = block(bi, bj);
                if (b.values.empty()) continue;
                for (int64_t c = 0; c < x.cols(); ++c)
                    for (int64_t i = 0; i < b.rows(); ++i) {
                        T s = 0;
                        for (int32_t k = b.rowptr[(size_t)i]; k < b.rowptr[(size_t)i + 1]; ++k) s += b.values[(size_t)k] * x((bj ? c0 : 0) + b.colidx[(size_t)k], c);
                        y((bi ? r0 : 0) + i, c) += s;
                    }
            }
        return y;
    }
   private:
    std::array<SpMatrix<T>, 4> blocks_;
    int64_t rows_ = 0, cols_ = 0;
};
// an n x m sparse matrix without entries (a zero block)
template <typename T> SpMatrix<T> zero_block(int64_t rows, int64_t cols) {
    SpMatrix<T> z;
    z.n_rows = rows, z.n_cols = cols, z.rowptr.assign((size_t)rows + 1, 0);
    return z;
}

// ---- Kronecker(A, B) (kronecker_product.h:56-80) --------------------------------------------------------------------------------------------------
// Kronecker(T, S), T dense q x q and S sparse n x n, is a LAZY expression: nothing is multiplied out.  Products add, subtract and scale to a KroneckerSum
// sum_k T_k (x) S_k, which PDE::KroneckerSolver::compute() hands to the device factor by factor (fdapde_kron_compute); eval() gives the explicit sparse
// matrix the reference's expression evaluates to (q n rows, entry (r n + i, s n + j) = sum_k T_k(r, s) S_k(i, j), sorted columns, entries of a term
// whose T_k(r, s) is an exact zero not stored).  Every factor is copied into the expression.
class KroneckerSum;
class KroneckerProduct {
   public:
    KroneckerProduct(const DMatrix<double>& t, const SpMatrix<double>& s) : T(t), S(s) {
        if (t.rows() != t.cols() || t.rows() < 1) throw std::runtime_error("Kronecker: the dense factor must be square");
        if (s.rows() != s.cols()) throw std::runtime_error("Kronecker: the sparse factor must be square");
    }
    int64_t rows() const { return T.rows() * S.rows(); }
    int64_t cols() const { return rows(); }
    inline SpMatrix<double> eval() const;
    DMatrix<double> T;
    SpMatrix<double> S;
};
inline KroneckerProduct Kronecker(const DMatrix<double>& t, const SpMatrix<double>& s) { return KroneckerProduct(t, s); }
// dense (x) dense, evaluated at once (host)
inline DMatrix<double> Kronecker(const DMatrix<double>& a, const DMatrix<double>& b) {
    DMatrix<double> c(a.rows() * b.rows(), a.cols() * b.cols());
    for (int64_t ja = 0; ja < a.cols(); ++ja)
        for (int64_t jb = 0; jb < b.cols(); ++jb)
            for (int64_t ia = 0; ia < a.rows(); ++ia)
                for (int64_t ib = 0; ib < b.rows(); ++ib) c(ia * b.rows() + ib, ja * b.cols() + jb) = a(ia, ja) * b(ib, jb);
    return c;
}

class KroneckerSum {
   public:
    KroneckerSum() = default;
    KroneckerSum(const KroneckerProduct& p) : terms_ {p} { }   // (a single product is a sum of one term)
    const std::vector<KroneckerProduct>& terms() const { return terms_; }
    int64_t time_size() const { return terms_.empty() ? 0 : terms_[0].T.rows(); }
    int64_t space_size() const { return terms_.empty() ? 0 : terms_[0].S.rows(); }
    int64_t rows() const { return time_size() * space_size(); }
    int64_t cols() const { return rows(); }
    KroneckerSum& operator+=(const KroneckerSum& o) {
        if (&o == this) return *this += KroneckerSum(o);   // (a += a: the loop below would walk the vector it grows)
        for (const KroneckerProduct& p : o.terms_) {
            if (!terms_.empty() && (p.T.rows() != time_size() || p.S.rows() != space_size())) throw std::runtime_error("KroneckerSum: the terms' factors differ in size");
            terms_.push_back(p);
        }
        return *this;
    }
    KroneckerSum& operator*=(double s) {
        for (KroneckerProduct& p : terms_)
            for (int64_t i = 0; i < p.T.size(); ++i) p.T.data()[i] *= s;
        return *this;
    }
    // the explicit matrix
    SpMatrix<double> eval() const {
        const int64_t q = time_size(), n = space_size();
        SpMatrix<double> a;
        a.n_rows = a.n_cols = q * n;
        a.rowptr.assign((size_t)(q * n) + 1, 0);
        std::vector<std::pair<int32_t, double>> row;
        for (int64_t r = 0; r < q; ++r)
            for (int64_t i = 0; i < n; ++i) {
                row.clear();
                for (const KroneckerProduct& p : terms_)
                    for (int64_t s = 0; s < q; ++s) {
                        const double t = p.T(r, s);
                        if (t == 0.0) continue;
                        for (int32_t k = p.S.rowptr[(size_t)i]; k < p.S.rowptr[(size_t)i + 1]; ++k)
                            row.emplace_back((int32_t)(s * n + p.S.colidx[(size_t)k]), t * p.S.values[(size_t)k]);
                    }
                std::stable_sort(row.begin(), row.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
                for (size_t k = 0; k < row.size(); ++k) {
                    if (k > 0 && row[k].first == row[k - 1].first) a.values.back() += row[k].second;   // (the terms in the order they were added)
                    else a.colidx.push_back(row[k].first), a.values.push_back(row[k].second);
                }
                a.rowptr[(size_t)(r * n + i) + 1] = (int32_t)a.colidx.size();
            }
        return a;
    }
   private:
    std::vector<KroneckerProduct> terms_;
};
inline SpMatrix<double> KroneckerProduct::eval() const { return KroneckerSum(*this).eval(); }
inline KroneckerSum operator+(KroneckerSum a, const KroneckerSum& b) { return a += b; }
inline KroneckerSum operator-(KroneckerSum a, KroneckerSum b) { return a += (b *= -1.0); }
inline KroneckerSum operator*(double s, KroneckerSum a) { return a *= s; }
inline KroneckerSum operator*(KroneckerSum a, double s) { return a *= s; }
inline KroneckerSum operator-(KroneckerSum a) { return a *= -1.0; }
inline KroneckerSum operator+(const KroneckerProduct& a, const KroneckerProduct& b) { return KroneckerSum(a) += KroneckerSum(b); }
inline KroneckerSum operator-(const KroneckerProduct& a, const KroneckerProduct& b) { return KroneckerSum(a) += (KroneckerSum(b) *= -1.0); }
inline KroneckerSum operator*(double s, const KroneckerProduct& a) { return KroneckerSum(a) *= s; }
inline KroneckerSum operator*(const KroneckerProduct& a, double s) { return KroneckerSum(a) *= s; }
inline KroneckerSum operator-(const KroneckerProduct& a) { return KroneckerSum(a) *= -1.0; }

// ---- small dense LU with partial pivoting (the DenseSolver of SMW; q x q) ----------------------------------------------
class PartialPivLU {
   public:
    void compute(const DMatrix<double>& a) {
        if (a.rows() != a.cols()) throw std::runtime_error("PartialPivLU: matrix must be square");
        n_ = a.rows(), lu_ = a, piv_.resize((size_t)n_);
        for (int64_t k = 0; k < n_; ++k) {
            int64_t p = k;
            for (int64_t i = k + 1; i < n_; ++i)
                if (std::fabs(lu_(i, k)) > std::fabs(lu_(p, k))) p = i;
            piv_[(size_t)k] = p;
            if (p != k)
                for (int64_t j = 0; j < n_; ++j) std::swap(lu_(k, j), lu_(p, j));
            if (lu_(k, k) == 0.0) throw std::runtime_error("PartialPivLU: singular matrix");
            for (int64_t i = k + 1; i < n_; ++i) {
                lu_(i, k) /= lu_(k, k);
                for (int64_t j = k + 1; j < n_; ++j) lu_(i, j) -= lu_(i, k) * lu_(k, j);
            }
        }
    }
    DMatrix<double> solve(const DMatrix<double>& b) const {
        if (b.rows() != n_) throw std::runtime_error("PartialPivLU: right-hand side has the wrong number of rows");
        DMatrix<double> x = b;
        for (int64_t c = 0; c < x.cols(); ++c) {
            for (int64_t k = 0; k < n_; ++k) std::swap(x(k, c), x(piv_[(size_t)k], c));
            for (int64_t i = 1; i < n_; ++i)
                for (int64_t j = 0; j < i; ++j) x(i, c) -= lu_(i, j) * x(j, c);
            for (int64_t i = n_ - 1; i >= 0; --i) {
                for (int64_t j = i + 1; j < n_; ++j) x(i, c) -= lu_(i, j) * x(j, c);
                x(i, c) /= lu_(i, i);
            }
        }
        return x;
    }
   private:
    int64_t n_ = 0;
    DMatrix<double> lu_;
    std::vector<int64_t> piv_;
};

// ---- Sherman-Morrison-Woodbury (same call signature as fdaPDE/linear_algebra/smw.h:38-59) -----------------------------
//   (A + U C V) x = b,  invC = C^{-1} supplied:   x = W_b - W_U (C^{-1} + V W_U)^{-1} (V W_b),   [W_b | W_U] = A^{-1} [b | U]
// ONE pass through the sparse solver: the m columns of b and the q columns of U go to the device as one (m + q)-column
// right-hand side: the columns of a small system run side by side in one persistent launch, those of a large one share every sweep over
// the matrix (fdapde_lin_solve batches 8 / 4 columns per multi-RHS CG, kernels_multirhs.h).  The correction A^{-1} U t of the formula is W_U t -- a dense n x q by q x m product on data already
// there, not another sparse solve (the reference performs three separate solves: b, U, and U t).
template <typename SparseSolver, typename DenseSolver = PartialPivLU> struct SMW {
    SMW() = default;
    DMatrix<double> solve(const SparseSolver& invA, const DMatrix<double>& U, const DMatrix<double>& invC, const DMatrix<double>& V,
                          const DMatrix<double>& b) {
        const int64_t n = b.rows(), m = b.cols(), q = U.cols();
        if (U.rows() != n || V.cols() != n || V.rows() != q || invC.rows() != q || invC.cols() != q)
            throw std::runtime_error("SMW: shapes of U, C^{-1}, V, b do not fit");
        DMatrix<double> rhs(n, m + q);
        std::copy(b.data(), b.data() + n * m, rhs.data());
        std::copy(U.data(), U.data() + n * q, rhs.data() + n * m);
        const DMatrix<double> W = invA.solve(rhs);                 // the only sparse solve: n x (m + q)
        // small dense part: S = C^{-1} + V W_U (q x q),  z = V W_b (q x m)
        DMatrix<double> S = invC, z(q, m, 0.0);
        for (int64_t c = 0; c < q + m; ++c) {
            const double* w = W.data() + n * c;                    // column c of W: first the m columns of b, then U's
            for (int64_t r = 0; r < q; ++r) {
                double acc = 0;
                for (int64_t i = 0; i < n; ++i) acc += V(r, i) * w[i];
                if (c < m) z(r, c) = acc;
                else S(r, c - m) += acc;
            }
        }
        DenseSolver dense;
        dense.compute(S);
        const DMatrix<double> t = dense.solve(z);                  // q x m
        DMatrix<double> x(n, m);
        for (int64_t c = 0; c < m; ++c) {
            double* xc = x.data() + n * c;
            std::copy(W.data() + n * c, W.data() + n * (c + 1), xc);
            for (int64_t k = 0; k < q; ++k) {
                const double tk = t(k, c);
                const double* wu = W.data() + n * (m + k);
                for (int64_t i = 0; i < n; ++i) xc[i] -= wu[i] * tk;
            }
        }
        return x;
    }
};

}   // namespace amd
}   // namespace fdapde

#endif
