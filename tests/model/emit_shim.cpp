// emit_shim.cpp -- TEST INFRASTRUCTURE ONLY: exposes the host emitter's number formatting and the text of one pair
// (lz-ani_amd/host/emit.h) to the Python tests.
#include "../../lz-ani_amd/host/emit.h"
extern "C" int host_format_real(double v, int prec, char* out) { return (int)host::real_to_chars(v, out, prec); }

// One pair of the genomes "A" (id 0, printed length la) and "B" (id 1, lb), `complete` columns: x = result of (ref A, query B),
// y = result of (ref B, query A); minima: the five of an --out-filter, or null for none.  The text by the table route (a
// two-genome PairTable through format_row) into by_table, and by the record route (a lzani_kept_pair with kept_lines
// through format_kept) into by_record, both 0-terminated and at most cap bytes.  Returns the `lines` of the table route's record.
extern "C" uint32_t host_format_pair(const int32_t* x, const int32_t* y, uint32_t la, uint32_t lb, const double* minima, int in_percent,
                                     uint32_t kept_lines, char* by_table, char* by_record, size_t cap)
{
    using namespace host;
    std::vector<Genome> g(2);
    g[0].name = "A"; g[1].name = "B";
    const std::vector<uint32_t> len = {la, lb};
    const lzani_result X{x[0], x[1], x[2]}, Y{y[0], y[1], y[2]};
    EmitParams ep;
    ep.in_percent = in_percent != 0;
    for (const auto& c : split(comp_metas().at("complete"), ',')) ep.comps.push_back(comp_names().at(c));
    ep.filtered = minima != nullptr;
    if (minima) ep.filter = lzani_out_filter{minima[0], minima[1], minima[2], minima[3], minima[4]};
    PairTable T;
    T.init_dense(2);
    T.res[0] = X; T.res[1] = Y;                              // row 0: query 1; row 1: query 0
    std::string t, r;
    format_row(g, len, T, ep, 0, t);
    format_kept(g, len, ep, lzani_kept_pair{0, 1, X, Y, kept_lines}, r);
    if (t.size() + 1 > cap || r.size() + 1 > cap) return 0xFFFFFFFFu;
    memcpy(by_table, t.c_str(), t.size() + 1);
    memcpy(by_record, r.c_str(), r.size() + 1);
    return make_record(len, ep, 0, 1, X, Y).lines;
}
