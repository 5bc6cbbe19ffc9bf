// BMat.h -- spECK::BMat: matOut = bmat(grid): a device CSR assembled from a grid of device CSR blocks, an absent cell a zero
// block; row i of block row g is the concatenation, in ascending block column, of row i of its blocks, column ids shifted
// by their block column's origin, values bit for bit.  spECK::VStack, HStack and BlockDiag are grids of one column, one
// row and the diagonal.  No reference counterpart.  Instantiated for float and double values; see speck_bmat_f64 in
// speck_c_api.h for the contract.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "dCSR.h"
#include "spECKConfig.h"

namespace spECK {
template <typename DataType>
struct BMatCell {
    uint32_t block_row, block_col;
    const dCSR<DataType>* M;
};

// rowSizes / colSizes: empty, or the height of every block row / the width of every block column (needed for a line
// without a block).  A refusal throws and leaves matOut as it was.
template <typename DataType>
void BMat(const std::vector<BMatCell<DataType>>& cells, uint32_t blockRows, uint32_t blockCols, dCSR<DataType>& matOut, spECKConfig& config,
          const std::vector<uint64_t>& rowSizes = {}, const std::vector<uint64_t>& colSizes = {}, speck_bmat_info* info = nullptr)
{
    if ((!rowSizes.empty() && rowSizes.size() != blockRows) || (!colSizes.empty() && colSizes.size() != blockCols))
        throw std::runtime_error("spECK::BMat: the sizes must name every line of the grid");
    std::vector<speck_dcsr> raw(cells.size());
    std::vector<speck_bmat_block> blocks(cells.size());
    for (size_t k = 0; k < cells.size(); ++k) {
        if (!cells[k].M) throw std::runtime_error("spECK::BMat: a cell without a matrix");
        raw[k] = cells[k].M->raw();
        blocks[k] = speck_bmat_block{cells[k].block_row, cells[k].block_col, &raw[k]};
    }
    const speck_bmat_params params{blockRows, blockCols, (uint32_t)cells.size(), blocks.empty() ? nullptr : blocks.data(),
                                   rowSizes.empty() ? nullptr : rowSizes.data(), colSizes.empty() ? nullptr : colSizes.data()};
    speck_dcsr c = matOut.raw();
    const int rc = sizeof(DataType) == 8 ? speck_bmat_f64(config.handle, &params, &c, info) : speck_bmat_f32(config.handle, &params, &c, info);
    matOut.adopt(c);  // (on an error `c` comes back as it went in)
    if (rc != SPECK_OK) throw std::runtime_error(std::string("spECK::BMat: ") + speck_status_string(rc));
}

template <typename DataType>
void VStack(const std::vector<const dCSR<DataType>*>& mats, dCSR<DataType>& matOut, spECKConfig& config, speck_bmat_info* info = nullptr)
{
    std::vector<BMatCell<DataType>> cells;
    for (size_t g = 0; g < mats.size(); ++g) cells.push_back({(uint32_t)g, 0u, mats[g]});
    BMat(cells, (uint32_t)mats.size(), 1u, matOut, config, {}, {}, info);
}

template <typename DataType>
void HStack(const std::vector<const dCSR<DataType>*>& mats, dCSR<DataType>& matOut, spECKConfig& config, speck_bmat_info* info = nullptr)
{
    std::vector<BMatCell<DataType>> cells;
    for (size_t q = 0; q < mats.size(); ++q) cells.push_back({0u, (uint32_t)q, mats[q]});
    BMat(cells, 1u, (uint32_t)mats.size(), matOut, config, {}, {}, info);
}

template <typename DataType>
void BlockDiag(const std::vector<const dCSR<DataType>*>& mats, dCSR<DataType>& matOut, spECKConfig& config, speck_bmat_info* info = nullptr)
{
    std::vector<BMatCell<DataType>> cells;
    for (size_t i = 0; i < mats.size(); ++i) cells.push_back({(uint32_t)i, (uint32_t)i, mats[i]});
    BMat(cells, (uint32_t)mats.size(), (uint32_t)mats.size(), matOut, config, {}, {}, info);
}
}  // namespace spECK
