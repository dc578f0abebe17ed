// pf_file.cpp — C ABI over the host metadata parser (pf_meta.cpp): open a file, read its
// footer (ParquetFileReader.open, ParquetReader.java:120), expose leaf columns in schema order
// (ParquetReader.java:126-128) and build pf_chunk_desc for a row group's chunks
// (readNextRowGroup, ParquetReader.java:183). No GPU calls.
#include <cerrno>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "pf_host.h"
#include "pfloor.h"

namespace {
thread_local std::string f_err;
int ferr(int code, const std::string& m) { f_err = m; return code; }
}  // namespace

struct pf_file {
    FILE* fp = nullptr;
    uint64_t size = 0;
    pf::FileMeta meta;
    std::map<std::pair<int, int>, std::vector<pf_page_desc>> pages;
    std::map<std::pair<int, int>, pf::ColumnIndexMeta> column_indexes;
    std::map<std::pair<int, int>, std::vector<pf_page_desc>> row_pages;   // pf_file_chunk_desc_rows (its own arrays)
};

extern "C" {

const char* pf_file_last_error(void) { return f_err.c_str(); }

int pf_file_open(const char* path, pf_file** out) {
    if (!path || !out) return ferr(PF_ERR_INVALID_ARG, "null arg");
    *out = nullptr;
    FILE* fp = std::fopen(path, "rb");
    if (!fp) return ferr(PF_ERR_IO, std::string("cannot open ") + path + ": " + std::strerror(errno));
    auto* f = new pf_file;
    f->fp = fp;
    std::fseek(fp, 0, SEEK_END);
    f->size = uint64_t(std::ftell(fp));
    try {
        if (f->size < 12) throw pf::MetaError("file too small to be parquet");
        uint8_t tail[8], head[4];
        std::fseek(fp, 0, SEEK_SET);
        if (std::fread(head, 1, 4, fp) != 4) throw pf::MetaError("read error");
        std::fseek(fp, long(f->size - 8), SEEK_SET);
        if (std::fread(tail, 1, 8, fp) != 8) throw pf::MetaError("read error");
        if (std::memcmp(head, "PAR1", 4) || std::memcmp(tail + 4, "PAR1", 4)) throw pf::MetaError("not a parquet file (magic)");
        uint32_t flen = uint32_t(tail[0]) | uint32_t(tail[1]) << 8 | uint32_t(tail[2]) << 16 | uint32_t(tail[3]) << 24;
        if (uint64_t(flen) + 12 > f->size) throw pf::MetaError("corrupt footer length");
        std::vector<uint8_t> foot(flen);
        std::fseek(fp, long(f->size - 8 - flen), SEEK_SET);
        if (flen && std::fread(foot.data(), 1, flen, fp) != flen) throw pf::MetaError("read error");
        f->meta.parse_footer(foot.data(), foot.size());
    } catch (const std::exception& e) {
        std::fclose(fp);
        delete f;
        return ferr(PF_ERR_IO, e.what());
    }
    *out = f;
    return PF_OK;
}

int pf_file_close(pf_file* f) {
    if (f) { if (f->fp) std::fclose(f->fp); delete f; }
    return PF_OK;
}

int pf_file_num_row_groups(pf_file* f, int* out) { if (!f || !out) return PF_ERR_INVALID_ARG; *out = int(f->meta.row_groups.size()); return PF_OK; }
int pf_file_num_columns(pf_file* f, int* out) { if (!f || !out) return PF_ERR_INVALID_ARG; *out = int(f->meta.leaves.size()); return PF_OK; }
int pf_file_num_rows(pf_file* f, int64_t* out) { if (!f || !out) return PF_ERR_INVALID_ARG; *out = f->meta.num_rows; return PF_OK; }
const char* pf_file_created_by(pf_file* f) { return f ? f->meta.created_by.c_str() : ""; }

int pf_file_column_meta(pf_file* f, int column, pf_column_meta* out) {
    if (!f || !out || column < 0 || column >= int(f->meta.leaves.size())) return ferr(PF_ERR_INVALID_ARG, "bad column");
    const pf::LeafMeta& L = f->meta.leaves[column];
    out->path = L.path.c_str();
    out->top_name = L.top.c_str();
    out->physical_type = L.physical_type; out->type_length = L.type_length;
    out->max_def = L.max_def; out->max_rep = L.max_rep;
    out->repeated_def = L.repeated_def; out->list_null_def = L.list_null_def;
    out->converted_type = L.converted_type; out->logical_type = L.logical_type;
    out->scale = L.scale; out->precision = L.precision;
    return PF_OK;
}

int pf_file_row_group_rows(pf_file* f, int rg, int64_t* out) {
    if (!f || !out || rg < 0 || rg >= int(f->meta.row_groups.size())) return ferr(PF_ERR_INVALID_ARG, "bad row group");
    *out = f->meta.row_groups[rg].num_rows;
    return PF_OK;
}

int pf_file_chunk_range(pf_file* f, int rg, int col, uint64_t* start, uint64_t* size) {
    if (!f || !start || !size || rg < 0 || rg >= int(f->meta.row_groups.size()) || col < 0 ||
        col >= int(f->meta.leaves.size()))
        return ferr(PF_ERR_INVALID_ARG, "bad index");
    const pf::ChunkMeta& m = f->meta.row_groups[rg].columns[col];
    if (m.num_values == 0) { *start = 0; *size = 0; return PF_OK; }
    int64_t s = m.start();
    if (s < 4 || m.total_compressed < 0 || uint64_t(s) + uint64_t(m.total_compressed) > f->size)
        return ferr(PF_ERR_IO, "column chunk outside the file");
    *start = uint64_t(s);
    *size = uint64_t(m.total_compressed);
    return PF_OK;
}

int pf_file_chunk_bloom(pf_file* f, int rg, int col, int64_t* offset, int32_t* length) {
    if (!f || !offset || !length || rg < 0 || rg >= int(f->meta.row_groups.size()) || col < 0 ||
        col >= int(f->meta.leaves.size()))
        return ferr(PF_ERR_INVALID_ARG, "bad index");
    const pf::ChunkMeta& m = f->meta.row_groups[rg].columns[col];
    *offset = -1;
    *length = -1;
    if (m.bloom_offset == -1 && m.bloom_length == -1) return PF_OK;
    const bool has_len = m.bloom_length != -1;
    if (m.bloom_offset < 4 || uint64_t(m.bloom_offset) >= f->size ||
        (has_len && (m.bloom_length < 0 || m.bloom_length > INT32_MAX || uint64_t(m.bloom_offset) + uint64_t(m.bloom_length) > f->size)))
        return ferr(PF_ERR_IO, "Bloom filter outside the file");
    *offset = m.bloom_offset;
    if (has_len) *length = int32_t(m.bloom_length);
    return PF_OK;
}

int pf_file_chunk_index_ranges(pf_file* f, int rg, int col, int64_t* ci_off, int32_t* ci_len, int64_t* oi_off, int32_t* oi_len) {
    if (!f || !ci_off || !ci_len || !oi_off || !oi_len || rg < 0 || rg >= int(f->meta.row_groups.size()) || col < 0 ||
        col >= int(f->meta.leaves.size()))
        return ferr(PF_ERR_INVALID_ARG, "bad index");
    const pf::ChunkMeta& m = f->meta.row_groups[rg].columns[col];
    *ci_off = *oi_off = -1;
    *ci_len = *oi_len = -1;
    auto range = [&](int64_t off, int64_t len, int64_t* o, int32_t* l) {
        if (off == -1 && len == -1) return true;
        if (off < 4 || len < 0 || len > INT32_MAX || uint64_t(off) + uint64_t(len) > f->size) return false;
        *o = off;
        *l = int32_t(len);
        return true;
    };
    if (!range(m.ci_offset, m.ci_length, ci_off, ci_len) || !range(m.oi_offset, m.oi_length, oi_off, oi_len))
        return ferr(PF_ERR_IO, "page index outside the file");
    return PF_OK;
}

namespace {
// The bytes of a chunk's index struct (which: 0 ColumnIndex, 1 OffsetIndex); PF_ERR_STATE when it has none.
int index_bytes(pf_file* f, int rg, int col, int which, std::vector<uint8_t>& buf) {
    int64_t off[2];
    int32_t len[2];
    int rc = pf_file_chunk_index_ranges(f, rg, col, &off[0], &len[0], &off[1], &len[1]);
    if (rc) return rc;
    if (off[which] < 0) return ferr(PF_ERR_STATE, which ? "the chunk has no OffsetIndex" : "the chunk has no ColumnIndex");
    buf.resize(size_t(len[which]));
    return pf_file_read(f, uint64_t(off[which]), uint64_t(len[which]), buf.data());
}
}  // namespace

int pf_file_offset_index(pf_file* f, int rg, int col, pf_page_location* out, int cap, int* n) {
    if (!n || cap < 0 || (cap > 0 && !out)) return ferr(PF_ERR_INVALID_ARG, "null arg");
    std::vector<uint8_t> buf;
    int rc = index_bytes(f, rg, col, 1, buf);
    if (rc) return rc;
    std::vector<pf_page_location> locs;
    try {
        pf::parse_offset_index(buf.data(), buf.size(), locs);
    } catch (const std::exception& e) {
        return ferr(PF_ERR_CORRUPT_PAGE, e.what());
    }
    if (locs.size() > size_t(INT32_MAX)) return ferr(PF_ERR_CORRUPT_PAGE, "too many page locations");
    *n = int(locs.size());
    for (int i = 0; i < *n && i < cap; i++) out[i] = locs[size_t(i)];
    return *n > cap ? ferr(PF_ERR_CAPACITY, "page location buffer too small") : PF_OK;
}

int pf_file_column_index(pf_file* f, int rg, int col, pf_column_index* out) {
    if (!out) return ferr(PF_ERR_INVALID_ARG, "null arg");
    std::vector<uint8_t> buf;
    int rc = index_bytes(f, rg, col, 0, buf);
    if (rc) return rc;
    pf::ColumnIndexMeta ci;
    try {
        pf::parse_column_index(buf.data(), buf.size(), ci);
    } catch (const std::exception& e) {
        return ferr(PF_ERR_CORRUPT_PAGE, e.what());
    }
    pf::ColumnIndexMeta& k = f->column_indexes[{rg, col}];
    k = std::move(ci);
    if (k.null_pages.empty()) k.null_pages.push_back(0);   // never a null pointer for an index that exists
    if (k.values.empty()) k.values.push_back(0);
    out->n_pages = int32_t((k.value_off.size() - 1) / 2);
    out->boundary_order = k.boundary_order;
    out->null_pages = k.null_pages.data();
    out->null_counts = k.has_null_counts ? k.null_counts.data() : nullptr;
    out->values = k.values.data();
    out->value_off = k.value_off.data();
    return PF_OK;
}

int pf_file_read(pf_file* f, uint64_t offset, uint64_t size, void* dst) {
    if (!f || (!dst && size)) return ferr(PF_ERR_INVALID_ARG, "null arg");
    if (offset + size > f->size) return ferr(PF_ERR_IO, "read past end of file");
    if (!size) return PF_OK;
    if (std::fseek(f->fp, long(offset), SEEK_SET) != 0) return ferr(PF_ERR_IO, "seek failed");
    if (std::fread(dst, 1, size, f->fp) != size) return ferr(PF_ERR_IO, "short read");
    return PF_OK;
}

int pf_file_chunk_desc(pf_file* f, int rg, int col, uint64_t chunk_offset_in_buffer, pf_chunk_desc* d) {
    if (!d) return ferr(PF_ERR_INVALID_ARG, "null desc");
    uint64_t start, size;
    int rc = pf_file_chunk_range(f, rg, col, &start, &size);
    if (rc) return rc;
    const pf::ChunkMeta& m = f->meta.row_groups[rg].columns[col];
    const pf::LeafMeta& L = f->meta.leaves[col];
    auto& pages = f->pages[{rg, col}];
    try {
        std::vector<uint8_t> buf(size);
        rc = pf_file_read(f, start, size, buf.data());
        if (rc) return rc;
        if (m.num_values > 0) pf::FileMeta::walk_pages(buf.data(), buf.size(), m, pages);
        else pages.clear();
    } catch (const std::exception& e) {
        return ferr(PF_ERR_CORRUPT_PAGE, e.what());
    }
    std::memset(d, 0, sizeof(*d));
    d->physical_type = L.physical_type;
    d->type_length = L.type_length;
    d->max_def = L.max_def;
    d->max_rep = L.max_rep;
    d->repeated_def = L.repeated_def;
    d->list_null_def = L.list_null_def;
    d->codec = m.codec;
    d->n_pages = int32_t(pages.size());
    d->pages = pages.empty() ? nullptr : pages.data();
    d->chunk_offset = chunk_offset_in_buffer;
    d->chunk_size = size;
    d->num_rows = f->meta.row_groups[rg].num_rows;
    return PF_OK;
}

int pf_file_chunk_desc_rows(pf_file* f, int rg, int col, int64_t row_lo, int64_t row_hi, uint64_t offset_in_buffer,
                            pf_chunk_desc* d, pf_chunk_rows* rows) {
    if (!d || !rows) return ferr(PF_ERR_INVALID_ARG, "null arg");
    uint64_t start, size;
    int rc = pf_file_chunk_range(f, rg, col, &start, &size);
    if (rc) return rc;
    const int64_t n_rows = f->meta.row_groups[rg].num_rows;
    if (row_lo < 0 || row_lo > row_hi || row_hi > n_rows) return ferr(PF_ERR_INVALID_ARG, "row range outside the row group");
    int64_t ci_off, oi_off;
    int32_t ci_len, oi_len;
    rc = pf_file_chunk_index_ranges(f, rg, col, &ci_off, &ci_len, &oi_off, &oi_len);
    if (rc) return rc;
    const pf::ChunkMeta& m = f->meta.row_groups[rg].columns[col];
    const pf::LeafMeta& L = f->meta.leaves[col];
    std::memset(rows, 0, sizeof(*rows));
    if (oi_off < 0 || m.num_values <= 0) {   // no OffsetIndex: every page, the window does the rest
        rc = pf_file_chunk_desc(f, rg, col, offset_in_buffer, d);
        if (rc) return rc;
        for (int i = 0; i < d->n_pages; i++) rows->n_data_pages += d->pages[i].page_type != PF_PAGE_DICTIONARY;
        rows->skip_rows = row_lo;
        rows->take_rows = row_hi - row_lo;
        rows->data_start = start;
        rows->data_size = size;
        return PF_OK;
    }
    std::vector<pf_page_desc> built;   // swapped in on success: a failed call leaves the earlier descriptor's array alone
    int64_t covered = 0;
    try {
        std::vector<uint8_t> buf;
        buf.resize(size_t(oi_len));
        rc = pf_file_read(f, uint64_t(oi_off), uint64_t(oi_len), buf.data());
        if (rc) return rc;
        std::vector<pf_page_location> locs;
        pf::parse_offset_index(buf.data(), buf.size(), locs);
        const size_t np = locs.size();
        if (np == 0 || np > size_t(INT32_MAX)) throw pf::MetaError("page locations: none, or too many");
        uint64_t prev_end = start;
        for (size_t p = 0; p < np; p++) {
            const pf_page_location& a = locs[p];
            if (uint64_t(a.offset) < prev_end || uint64_t(a.offset) > start + size ||
                uint64_t(a.compressed_page_size) > start + size - uint64_t(a.offset))
                throw pf::MetaError("page location outside the chunk, or not increasing");
            prev_end = uint64_t(a.offset) + uint64_t(a.compressed_page_size);
            if (p == 0 ? a.first_row_index != 0 : a.first_row_index <= locs[p - 1].first_row_index)
                throw pf::MetaError("page location first_row_index not increasing from 0");
            if (a.first_row_index >= n_rows) throw pf::MetaError("page location first_row_index past the row group");
        }
        auto row_end = [&](size_t p) { return p + 1 < np ? locs[p + 1].first_row_index : n_rows; };
        rows->indexed = 1;
        rows->first_row = row_lo;
        rows->take_rows = row_hi - row_lo;
        size_t p0 = 0, p1 = 0;   // [p0, p1)
        if (row_lo < row_hi) {
            while (row_end(p0) <= row_lo) p0++;
            p1 = p0;
            while (p1 < np && locs[p1].first_row_index < row_hi) p1++;
            rows->first_page = int32_t(p0);
            rows->n_data_pages = int32_t(p1 - p0);
            rows->first_row = locs[p0].first_row_index;
            rows->skip_rows = row_lo - rows->first_row;
            rows->dict_start = start;
            rows->dict_size = uint64_t(locs[0].offset) - start;
            rows->data_start = uint64_t(locs[p0].offset);
            rows->data_size = uint64_t(locs[p1 - 1].offset) + uint64_t(locs[p1 - 1].compressed_page_size) - rows->data_start;
            covered = row_end(p1 - 1) - rows->first_row;
        }
        buf.resize(size_t(rows->dict_size + rows->data_size));
        if (rows->dict_size) {
            rc = pf_file_read(f, rows->dict_start, rows->dict_size, buf.data());
            if (rc) return rc;
            pf_page_desc pd;
            const size_t h = pf::read_page_header(buf.data(), size_t(rows->dict_size), pd);
            if (pd.page_type != PF_PAGE_DICTIONARY || int32_t(pd.compressed_size) < 0 ||
                uint64_t(h) + pd.compressed_size > rows->dict_size)
                throw pf::MetaError("no dictionary page before the first page location");
            pd.offset = h;
            built.push_back(pd);
        }
        if (rows->data_size) {
            rc = pf_file_read(f, rows->data_start, rows->data_size, buf.data() + rows->dict_size);
            if (rc) return rc;
        }
        for (size_t p = p0; p < p1; p++) {
            const uint64_t at = rows->dict_size + (uint64_t(locs[p].offset) - rows->data_start);
            const uint64_t cps = uint64_t(locs[p].compressed_page_size);
            pf_page_desc pd;
            const size_t h = pf::read_page_header(buf.data() + at, size_t(cps), pd);
            if (int32_t(pd.compressed_size) < 0 || uint64_t(h) + pd.compressed_size > cps)
                throw pf::MetaError("compressed_page_size shorter than the page");
            if (pd.page_type != PF_PAGE_DATA && pd.page_type != PF_PAGE_DATA_V2) throw pf::MetaError("page location of no data page");
            if (pd.num_values < 0) throw pf::MetaError("negative num_values");
            if (pd.page_type == PF_PAGE_DATA_V2) {
                if (pd.def_bytes < 0 || pd.rep_bytes < 0 || uint64_t(pd.def_bytes) + uint64_t(pd.rep_bytes) > pd.compressed_size ||
                    uint64_t(pd.def_bytes) + uint64_t(pd.rep_bytes) > pd.uncompressed_size)
                    throw pf::MetaError("v2 level lengths exceed page");
                if (int64_t(pd.num_rows) != row_end(p) - locs[p].first_row_index)
                    throw pf::MetaError("v2 num_rows disagrees with the OffsetIndex");
            }
            pd.offset = at + h;
            built.push_back(pd);
        }
    } catch (const std::exception& e) {
        return ferr(PF_ERR_CORRUPT_PAGE, e.what());
    }
    auto& pages = f->row_pages[{rg, col}];
    pages.swap(built);
    std::memset(d, 0, sizeof(*d));
    d->physical_type = L.physical_type;
    d->type_length = L.type_length;
    d->max_def = L.max_def;
    d->max_rep = L.max_rep;
    d->repeated_def = L.repeated_def;
    d->list_null_def = L.list_null_def;
    d->codec = m.codec;
    d->n_pages = int32_t(pages.size());
    d->pages = pages.empty() ? nullptr : pages.data();
    d->chunk_offset = offset_in_buffer;
    d->chunk_size = rows->dict_size + rows->data_size;
    d->num_rows = covered;
    return PF_OK;
}

}  // extern "C"
