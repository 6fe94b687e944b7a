/*
 * ref_dbow.cc -- driver that runs the reference's own Thirdparty/DBoW2 (FORB.cpp, BowVector.cpp, FeatureVector.cpp,
 * ScoringObject.cpp, TemplatedVocabulary.h, DUtils/Random.cpp, DUtils/Timestamp.cpp; compiled unmodified on the OpenCV
 * shim in cv_shim/) on a batch of cases, for tests/test_reference_pin_dbow_*.py.
 *
 *   ref_dbow REQUEST RESPONSE
 *
 * TEST INFRASTRUCTURE ONLY.  A standalone executable: it keeps the reference's code out of the test process.
 *
 * Reference behaviours this driver and its tests respect:
 *   - Missing file.  loadFromTextFile (TemplatedVocabulary.h:1338) never terminates on a file that cannot be opened: the
 *     stream never reaches eof and m_nodes grows until the process is killed.  The driver opens the file itself first and
 *     exits with status 2 when it cannot.  (Every caller also gives the process a timeout.)
 *   - Trailing newline.  The read-until-eof loop (:1378) turns the empty string after a final newline into one more
 *     node under the root whose descriptor is never written.  saveToTextFile ends the file with a newline.  The driver
 *     therefore hands loadFromTextFile a copy of the file without its trailing line ends (RESPONSE + ".voc", removed again);
 *     include/orbv.h documents that the product ignores empty lines.
 *   - Unbalanced trees.  transform(features, BowVector, FeatureVector, levelsup) declares its node id without a value (:1151, :1179) and
 *     the single-feature transform writes it only on reaching level L - levelsup (:1251), so for a feature whose leaf is
 *     shallower than that level the FeatureVector's node is indeterminate.  In the per-feature results the driver presets
 *     nid to NID_UNSET (0xFFFFFFFF); the tests compare node ids and FeatureVector entries only where the leaf is deep enough.
 *   - Node count.  loadFromTextFile reserves (k^(L+1) - 1)/(k - 1) nodes (:1370-1372) and keeps pointers into m_nodes in
 *     m_words; past the reservation they dangle.  The driver counts the file's node lines and exits with status 2 when there
 *     are more than that (k is at least 2: k = 1 divides by zero there).
 *   - A node is a leaf iff it has no children (Node::isLeaf), whatever the file's flag says; the flag only decides
 *     whether it gets a word id.  Case files keep the two in agreement.
 *
 * Request (little-endian): int32 magic 'DBWQ', int32 ncases, then per case int32 mode and
 *   LOAD:      int32 len + path.  The vocabulary becomes the current one of the following cases.
 *   TRANSFORM: int32 levelsup, n; n x 32 descriptor bytes
 *   SCORE:     int32 npairs; per pair int32 n1, n1 x uint32 ids, n1 x float64 values, int32 n2, ids, values
 *   CREATE:    int32 seed, k, L, weighting, scoring, nimages; per image int32 n + n x 32 bytes; int32 len + output path.
 *              DUtils::Random::SeedRandOnce(seed) acts once per process, so a request holds at most one CREATE.
 * Response: int32 magic 'DBWR', then per case int32 mode and
 *   LOAD:      int32 k, L, scoring, weighting, nnodes (root included), nwords; then per-node arrays over all nnodes:
 *              int32 parent, int32 isLeaf(), int32 word_id, float64 weight, 32 descriptor bytes (zeros for the root, which
 *              has none), int32 number of children; then all children lists concatenated, in order
 *   TRANSFORM: n x uint32 word id, n x float64 weight, n x uint32 node id (transform(feature, id, w, &nid, levelsup));
 *              then transform(features, bow, fv, levelsup): int32 nb, nb x uint32 ids, nb x float64 values;
 *              int32 nn, per node uint32 id, int32 count, count x uint32 feature indices
 *   SCORE:     npairs x float64 voc.score(v1, v2)
 *   CREATE:    int32 len + the bytes saveToTextFile wrote
 * float64 values travel as their bits.
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "DBoW2/FORB.h"
#include "DBoW2/TemplatedVocabulary.h"
#include "DUtils/Random.h"

typedef DBoW2::TemplatedVocabulary<DBoW2::FORB::TDescriptor, DBoW2::FORB> Voc;

class Probe : public Voc {
public:
    using Voc::m_nodes;
    using Voc::m_words;
    using Voc::transform;      /* the single-feature overload with nid and levelsup is protected */
};

enum { M_LOAD = 0, M_TRANSFORM = 1, M_SCORE = 2, M_CREATE = 3 };
static const uint32_t NID_UNSET = 0xFFFFFFFFu;

static const unsigned char *g_in, *g_in_end;
static FILE *g_out;
static std::string g_resp_path;

static void fail(const char *m) { std::fprintf(stderr, "ref_dbow: %s\n", m); std::exit(2); }
static void rd(void *p, size_t n)
{
    if ((size_t)(g_in_end - g_in) < n) fail("truncated request");
    if (n) std::memcpy(p, g_in, n);
    g_in += n;
}
static int32_t rd_i() { int32_t v; rd(&v, 4); return v; }
static std::string rd_s()
{
    const int n = rd_i();
    if (n < 0 || n > 4096) fail("bad string length");
    std::string s((size_t)n, '\0');
    rd(&s[0], (size_t)n);
    return s;
}
static void wr(const void *p, size_t n) { if (n && std::fwrite(p, 1, n, g_out) != n) fail("write failed"); }
static void wr_i(int32_t v) { wr(&v, 4); }
static void wr_u(uint32_t v) { wr(&v, 4); }
static void wr_d(double v) { wr(&v, 8); }

static std::string slurp(const std::string &path, const char *what)
{
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) fail(what);
    std::string s;
    char buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
    std::fclose(f);
    return s;
}

static std::vector<cv::Mat> rd_features(int n)
{
    if (n < 0) fail("bad feature count");
    std::vector<cv::Mat> v((size_t)n);
    for (int i = 0; i < n; i++) {
        v[i].create(1, 32, CV_8U);
        rd(v[i].ptr(), 32);
    }
    return v;
}

static void load(Probe &voc)
{
    const std::string path = rd_s();
    std::string text = slurp(path, "cannot open the vocabulary file");
    while (!text.empty() && (text[text.size() - 1] == '\n' || text[text.size() - 1] == '\r')) text.erase(text.size() - 1);
    int k = 0, L = 0;
    if (std::sscanf(text.c_str(), "%d %d", &k, &L) != 2 || k < 2 || k > 20 || L < 1 || L > 10) fail("bad vocabulary header");
    size_t lines = 0;
    for (size_t i = 0; i < text.size(); i++) lines += text[i] == '\n';      /* node lines: all but the header */
    const double reserved = (std::pow((double)k, (double)L + 1) - 1) / (k - 1);
    if ((double)lines + 1 > reserved) fail("more nodes than loadFromTextFile reserves for this k and L");
    const std::string tmp = g_resp_path + ".voc";
    FILE *f = std::fopen(tmp.c_str(), "wb");
    if (!f || std::fwrite(text.data(), 1, text.size(), f) != text.size() || std::fclose(f) != 0) fail("cannot write the vocabulary copy");
    const bool ok = voc.loadFromTextFile(tmp);
    std::remove(tmp.c_str());
    if (!ok) fail("loadFromTextFile refused the file");

    const int nn = (int)voc.m_nodes.size();
    wr_i(voc.getBranchingFactor()); wr_i(voc.getDepthLevels());
    wr_i((int)voc.getScoringType()); wr_i((int)voc.getWeightingType());
    wr_i(nn); wr_i((int)voc.m_words.size());
    for (int i = 0; i < nn; i++) wr_i(i ? (int32_t)voc.m_nodes[i].parent : 0);
    for (int i = 0; i < nn; i++) wr_i(voc.m_nodes[i].isLeaf() ? 1 : 0);
    for (int i = 0; i < nn; i++) wr_i((int32_t)voc.m_nodes[i].word_id);
    for (int i = 0; i < nn; i++) wr_d(voc.m_nodes[i].weight);
    for (int i = 0; i < nn; i++) {
        unsigned char z[32] = {0};
        const cv::Mat &d = voc.m_nodes[i].descriptor;
        if (!d.empty()) { if (d.cols != 32) fail("descriptor width"); std::memcpy(z, d.ptr(), 32); }
        wr(z, 32);
    }
    for (int i = 0; i < nn; i++) wr_i((int32_t)voc.m_nodes[i].children.size());
    for (int i = 0; i < nn; i++)
        for (size_t c = 0; c < voc.m_nodes[i].children.size(); c++) wr_u(voc.m_nodes[i].children[c]);
}

static void transform(const Probe &voc)
{
    const int levelsup = rd_i(), n = rd_i();
    const std::vector<cv::Mat> feat = rd_features(n);
    std::vector<uint32_t> wid((size_t)n), nid((size_t)n);
    std::vector<double> w((size_t)n);
    for (int i = 0; i < n; i++) {
        DBoW2::WordId id = 0;
        DBoW2::WordValue wt = 0;
        DBoW2::NodeId nd = NID_UNSET;
        voc.transform(feat[i], id, wt, &nd, levelsup);
        wid[i] = id; w[i] = wt; nid[i] = nd;
    }
    wr(wid.data(), (size_t)n * 4); wr(w.data(), (size_t)n * 8); wr(nid.data(), (size_t)n * 4);
    DBoW2::BowVector bow;
    DBoW2::FeatureVector fv;
    voc.transform(feat, bow, fv, levelsup);
    wr_i((int32_t)bow.size());
    for (DBoW2::BowVector::const_iterator it = bow.begin(); it != bow.end(); ++it) wr_u(it->first);
    for (DBoW2::BowVector::const_iterator it = bow.begin(); it != bow.end(); ++it) wr_d(it->second);
    wr_i((int32_t)fv.size());
    for (DBoW2::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it) {
        wr_u(it->first);
        wr_i((int32_t)it->second.size());
        for (size_t j = 0; j < it->second.size(); j++) wr_u(it->second[j]);
    }
}

static DBoW2::BowVector rd_bow()
{
    const int n = rd_i();
    if (n < 0) fail("bad BowVector size");
    std::vector<uint32_t> ids((size_t)n);
    std::vector<double> vals((size_t)n);
    rd(ids.data(), (size_t)n * 4); rd(vals.data(), (size_t)n * 8);
    DBoW2::BowVector v;
    for (int i = 0; i < n; i++) v.insert(v.end(), DBoW2::BowVector::value_type(ids[i], vals[i]));
    if ((int)v.size() != n) fail("BowVector ids are not distinct");
    return v;
}

static void score(const Probe &voc)
{
    const int np = rd_i();
    for (int p = 0; p < np; p++) {
        const DBoW2::BowVector a = rd_bow();
        const DBoW2::BowVector b = rd_bow();
        wr_d(voc.score(a, b));
    }
}

static void create()
{
    static bool created = false;
    if (created) fail("one CREATE per process (SeedRandOnce)");
    created = true;
    const int seed = rd_i(), k = rd_i(), L = rd_i(), weighting = rd_i(), scoring = rd_i(), nimg = rd_i();
    if (k < 2 || k > 20 || L < 1 || L > 10 || weighting < 0 || weighting > 3 || scoring < 0 || scoring > 5 || nimg < 1) fail("bad CREATE parameters");
    std::vector<std::vector<cv::Mat> > training((size_t)nimg);
    for (int i = 0; i < nimg; i++) training[i] = rd_features(rd_i());
    const std::string out = rd_s();
    DUtils::Random::SeedRandOnce(seed);
    Probe voc;
    voc.create(training, k, L, (DBoW2::WeightingType)weighting, (DBoW2::ScoringType)scoring);
    voc.saveToTextFile(out);
    const std::string text = slurp(out, "saveToTextFile wrote nothing");
    wr_i((int32_t)text.size());
    wr(text.data(), text.size());
}

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: ref_dbow REQUEST RESPONSE\n"); return 2; }
    const std::string req = slurp(argv[1], "cannot open the request");
    g_in = (const unsigned char *)req.data(); g_in_end = g_in + req.size();
    if (rd_i() != 0x51574244) fail("bad request magic");
    const int ncases = rd_i();
    g_resp_path = argv[2];
    g_out = std::fopen(argv[2], "wb");
    if (!g_out) fail("cannot open the response");
    wr_i(0x52574244);
    Probe voc;
    bool loaded = false;
    for (int c = 0; c < ncases; c++) {
        const int mode = rd_i();
        wr_i(mode);
        if (mode == M_LOAD) { load(voc); loaded = true; }
        else if (mode == M_CREATE) create();
        else if (!loaded) fail("TRANSFORM or SCORE before LOAD");
        else if (mode == M_TRANSFORM) transform(voc);
        else if (mode == M_SCORE) score(voc);
        else fail("unknown mode");
    }
    if (std::fclose(g_out) != 0) fail("cannot close the response");
    return 0;
}
