// pf_host.h — host-side metadata model (footer + page headers). Internal.
#pragma once
#include <cstdint>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "pfloor.h"

namespace pf {

struct MetaError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

struct ChunkMeta {
    int type = -1, codec = 0;
    int64_t num_values = 0, total_uncompressed = 0, total_compressed = 0;
    int64_t data_page_offset = 0, dictionary_page_offset = 0;
    bool has_dict = false;
    int64_t bloom_offset = -1, bloom_length = -1;   // ColumnMetaData 14 / 15 (-1: absent)
    int64_t oi_offset = -1, oi_length = -1;         // ColumnChunk 4 / 5: the OffsetIndex (-1: absent)
    int64_t ci_offset = -1, ci_length = -1;         // ColumnChunk 6 / 7: the ColumnIndex
    // ColumnChunkMetaData.getStartingPos(): the dictionary page offset when it precedes
    // the first data page, else the data page offset.
    int64_t start() const {
        if (has_dict && dictionary_page_offset > 0 && dictionary_page_offset < data_page_offset)
            return dictionary_page_offset;
        return data_page_offset;
    }
};

struct RowGroupMeta {
    int64_t num_rows = 0;
    std::vector<ChunkMeta> columns;
};

struct LeafMeta {
    std::string path, top;
    int physical_type = -1, type_length = 0, max_def = 0, max_rep = 0, repeated_def = 0, list_null_def = 0;
    int converted_type = -1, logical_type = 0;
    int scale = 0, precision = 0;
};

struct FileMeta {
    int64_t num_rows = 0;
    std::string created_by;
    std::vector<LeafMeta> leaves;
    std::vector<RowGroupMeta> row_groups;

    void parse_footer(const uint8_t* p, size_t n);
    static void walk_pages(const uint8_t* chunk, size_t size, const ChunkMeta& m, std::vector<pf_page_desc>& out);
};

// A chunk's ColumnIndex as pf_file_column_index returns it: page p's min is values[value_off[2p], value_off[2p+1]),
// its max values[value_off[2p+1], value_off[2p+2]).
struct ColumnIndexMeta {
    int boundary_order = 0;
    bool has_null_counts = false;
    std::vector<uint8_t> null_pages, values;
    std::vector<int64_t> null_counts;
    std::vector<uint32_t> value_off;
};
// Parse the Thrift compact structs at [p, p + n); unknown fields are skipped. MetaError when damaged (a varint or
// a length past the range, list lengths that disagree, a missing required field); never reads outside the range.
void parse_column_index(const uint8_t* p, size_t n, ColumnIndexMeta& out);
void parse_offset_index(const uint8_t* p, size_t n, std::vector<pf_page_location>& out);
// One Thrift compact PageHeader at [p, p + n): fills d (offset 0) and returns the header's length; MetaError when
// damaged. The reader and the limits (PF_THRIFT_MAX_NESTING) of FileMeta::walk_pages, which calls it per page.
size_t read_page_header(const uint8_t* p, size_t n, pf_page_desc& d);

// Statistics of a page or a chunk as the write path serialises them (parquet.thrift Statistics: 3 null_count,
// 5 max_value, 6 min_value; the legacy 1 max / 2 min only where `legacy` says so).
struct StatsOut {
    bool present = false;      // write the struct at all
    bool has_min_max = false, legacy = false;
    int64_t null_count = 0;
    std::string min, max;      // PLAIN bytes
};

// One page header of the write path (pf_write.cpp serialises it as a Thrift compact PageHeader).
struct PageHeaderOut {
    int32_t page_type = 0, uncompressed_size = 0, compressed_size = 0;
    int32_t num_values = 0, num_nulls = 0, num_rows = 0, encoding = 0, def_bytes = 0;
    bool is_compressed = true;
    bool has_crc = false;
    uint32_t crc = 0;          // PageHeader.crc (field 4): CRC-32 of the compressed_size bytes after the header
    StatsOut stats;            // DataPageHeaderV2.statistics (field 8)
};
void write_page_header(std::vector<uint8_t>& out, const PageHeaderOut& h);

}  // namespace pf
