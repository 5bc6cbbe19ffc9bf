// SpMMT.h -- spECK::TransposePlan and spECK::SpMMT: Y = alpha A^T X + beta Y on a device matrix with k right-hand sides,
// without transposing A.  A TransposePlan is the pattern of A sorted by column once (A's values are not read); SpMMT gathers
// the current values through it, so a training loop whose values change every step and whose pattern never does sorts
// once.  d_X (A.rows x k, indexed by the row inside A) and d_Y (A.cols x k) are ROW-MAJOR device arrays of doubles for both
// value types, with leading dimensions ldx >= k and ldy >= k.  Column c of Y is bit for bit what spECK::SpMM writes on
// spECK::Transpose(A); the plan is verified against A in every call, and a matrix with another pattern is refused with
// nothing of Y written.  A row-range view gives the partial sum of its rows.  No reference counterpart.
// Instantiated for float and double; see speck_spmm_t_f64 in speck_c_api.h for the contract.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>

#include "dCSR.h"
#include "spECKConfig.h"

namespace spECK {
// RAII over speck_tplan: movable, not copyable; several calls, streams and configs may use one plan
class TransposePlan {
public:
    TransposePlan() = default;
    template <typename DataType>
    explicit TransposePlan(const dCSR<DataType>& A, speck_tplan_info* info = nullptr)
    {
        speck_dcsr a = A.raw();
        const int rc = speck_tplan_create(nullptr, &a, &plan_, info);
        if (rc != SPECK_OK) throw std::runtime_error(std::string("spECK::TransposePlan: ") + speck_status_string(rc));
    }
    TransposePlan(const TransposePlan&) = delete;
    TransposePlan& operator=(const TransposePlan&) = delete;
    TransposePlan(TransposePlan&& o) noexcept : plan_(std::exchange(o.plan_, nullptr)) {}
    TransposePlan& operator=(TransposePlan&& o) noexcept
    {
        if (this != &o) {
            reset();
            plan_ = std::exchange(o.plan_, nullptr);
        }
        return *this;
    }
    ~TransposePlan() { reset(); }
    void reset()
    {
        (void)speck_tplan_destroy(plan_);
        plan_ = nullptr;
    }
    const speck_tplan* get() const { return plan_; }
    explicit operator bool() const { return plan_ != nullptr; }

private:
    speck_tplan* plan_ = nullptr;
};

template <typename DataType>
void SpMMT(const TransposePlan& plan, const dCSR<DataType>& A, const double* d_X, uint64_t ldx, uint32_t k, double* d_Y, uint64_t ldy,
           spECKConfig& config, double alpha = 1.0, double beta = 0.0, speck_spmm_t_info* info = nullptr)
{
    speck_dcsr a = A.raw();
    const int rc = sizeof(DataType) == 8 ? speck_spmm_t_f64(config.handle, plan.get(), alpha, &a, d_X, ldx, k, beta, d_Y, ldy, info)
                                         : speck_spmm_t_f32(config.handle, plan.get(), alpha, &a, d_X, ldx, k, beta, d_Y, ldy, info);
    if (rc != SPECK_OK) throw std::runtime_error(std::string("spECK::SpMMT: ") + speck_status_string(rc));
}

// float blocks (speck_spmm_t_f64_b32 / _f32_b32): ldx and ldy count floats; Y is bit for bit the result above on the
// widened blocks with the same plan, rounded to float once
template <typename DataType>
void SpMMT(const TransposePlan& plan, const dCSR<DataType>& A, const float* d_X, uint64_t ldx, uint32_t k, float* d_Y, uint64_t ldy,
           spECKConfig& config, double alpha = 1.0, double beta = 0.0, speck_spmm_t_info* info = nullptr)
{
    speck_dcsr a = A.raw();
    const int rc = sizeof(DataType) == 8 ? speck_spmm_t_f64_b32(config.handle, plan.get(), alpha, &a, d_X, ldx, k, beta, d_Y, ldy, info)
                                         : speck_spmm_t_f32_b32(config.handle, plan.get(), alpha, &a, d_X, ldx, k, beta, d_Y, ldy, info);
    if (rc != SPECK_OK) throw std::runtime_error(std::string("spECK::SpMMT: ") + speck_status_string(rc));
}
}  // namespace spECK
