// What the two translation units of the homology search share (wf_search.hip: the ungapped
// rule; wf_search_gap.hip: the gapped extension of its records): the device buffers kept in
// the mapper's state and the ungapped records of one chunk.
#pragma once

#include <string>
#include <vector>

#include "wf_internal.h"
#include "wf_mapstore.h"

namespace wf {

struct SearchState {
  MapBuf seq, off, soff, pk[2], nm[2], cnt, first, start, tmp, raw, ctr;
  MapBuf g_anchor, g_out;     // the gapped extension's anchors and results of one launch
};

struct SearchRec { int32_t contig, subject, minus, qstart, sstart, length, matches; };

// The ungapped records of the chunk, sorted by (contig, subject, minus,
// qstart, sstart, length).  When any seed slot exists, the chunk's bit planes (pk, nm of both
// strands) and `off` stay resident in st->search afterwards.
int search_records(MapState* st, const char* seq, const int64_t* off, int64_t n_subjects, const SearchRule& rule,
                   std::vector<SearchRec>* recs, SearchStats* stats, hipStream_t s, std::string* err);

}  // namespace wf
