// mcs_facade.hpp — header-only C++ host facade over the C ABI (include/mcs_c.h) with the reference's class names, so
// that cTracking / cLocalMapping / cLoopClosing compile against it unchanged in spirit:
//
//   MultiColSLAM::mdBRIEFextractorOct   include/mdBRIEFextractorOct.h:335-421 (13-argument ctor, operator(), getters)
//   MultiColSLAM::ORBextractor          include/cORBextractor.h:48-67 (the ORB-mode extractor behind its own constructor / operator())
//   MultiColSLAM::cORBmatcher           include/cORBmatcher.h:43-133 (brute-force and grid-window searches on flat views)
//   MultiColSLAM::cMultiCamSys_ / LoadMCS / cORBVocabulary / ComputeDistinctiveDescriptors   the callers either side of the path
//   MultiColSLAM::DescriptorDistance64[_Masked]   src/cORBmatcher.cpp:2438-2474
//   MultiColSLAM::cMultiKeyFrameDatabase<KF>     include/cMultiKeyFrameDatabase.h, src/cMultiKeyFrameDatabase.cpp (the inverted file on the device)
//
// OpenCV is not a dependency: minimal layout-compatible PODs stand in for cv::KeyPoint / cv::Mat / cv::Vec3d.  With
// -DMCS_WITH_OPENCV the adapters at the bottom accept the real types (cv::KeyPoint is 28 bytes, same layout).
// Link with -lmcs_hip.  No CPU fallback: every call needs a HIP device and throws std::runtime_error otherwise.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <list>
#include <map>
#include <set>
#include <sstream>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../mcs_c.h"

namespace MultiColSLAM {

struct KeyPoint { float ptx, pty, size, angle, response; int32_t octave, class_id; };   // == cv::KeyPoint, 28 B
static_assert(sizeof(KeyPoint) == 28 && sizeof(mcs_keypoint) == 28, "cv::KeyPoint layout");
struct Vec3d { double v[3]; };

struct Mat8u {   // CV_8UC1 matrix view / owner (rows x cols, step bytes per row)
	int rows = 0, cols = 0, step = 0;
	std::vector<uint8_t> store;
	uint8_t* data = nullptr;
	void create(int r, int c) { rows = r; cols = c; step = c; store.assign((size_t)r * c, 0); data = store.data(); }
	void release() { rows = cols = step = 0; store.clear(); data = nullptr; }
	bool empty() const { return rows == 0 || cols == 0; }
	const uint64_t* ptr64(int r) const { return reinterpret_cast<const uint64_t*>(data + (size_t)r * step); }
};

inline void mcs_throw(int rc) { if (rc != MCS_OK) throw std::runtime_error(std::string("libmcs_hip: ") + mcs_last_error()); }

class Context {
public:
	explicit Context(int device = 0, void* hipStream = nullptr) { mcs_throw(mcs_ctx_create(device, hipStream, &h)); }
	~Context() { mcs_ctx_destroy(h); }
	Context(const Context&) = delete;
	Context& operator=(const Context&) = delete;
	// A pipelined host (include/mcs_c.h: "Long transfers beside the step"): results leave on resultStream() through copyNarrow(), images arrive by hipMemcpyAsync on
	// transferStream(), a stream the library has probed to share a hardware queue with none of the streams the extraction runs on.
	void* resultStream() const { void* s = nullptr; mcs_throw(mcs_ctx_result_stream(h, &s)); return s; }
	void* transferStream(unsigned* conflicts = nullptr) const { void* s = nullptr; mcs_throw(mcs_ctx_transfer_stream(h, &s, conflicts)); return s; }
	unsigned streamConflicts(void* hipStream) const { unsigned m = 0; mcs_throw(mcs_ctx_stream_conflicts(h, hipStream, &m)); return m; }
	void copyNarrow(void* dst, const void* src, size_t bytes, void* hipStream, int workgroups = 2) const { mcs_throw(mcs_copy_narrow(h, dst, src, bytes, workgroups, hipStream)); }
	void synchronize() const { mcs_throw(mcs_ctx_synchronize(h)); }
	mcs_ctx* h = nullptr;
};

// cCamModelGeneral_ (include/cam_model_omni.h): calibration + level-0 mirror mask
struct cCamModelGeneral_ {
	mcs_ocam ocam{};
	Mat8u mirrorMask0;
	double GetWidth() const { return ocam.width; }
	double GetHeight() const { return ocam.height; }
	const Mat8u& GetMirrorMask(int) const { return mirrorMask0; }
};

class mdBRIEFextractorOct {
public:
	enum { HARRIS_SCORE = 0, FAST_SCORE = 1 };
	mdBRIEFextractorOct(Context& ctx, int _nfeatures = 1000, float _scaleFactor = 1.2f, int _nlevels = 8, int _edgeThreshold = 25,
	                    int _firstLevel = 0, int _scoreType = HARRIS_SCORE, int _patchSize = 32, int _fastThreshold = 20, bool _useAgast = false,
	                    int _fastAgastType = 2, bool _do_dBrief = false, bool _learnMasks = false, int _descSize = 32)
	    : ctx_(ctx), p_{_nfeatures, _scaleFactor, _nlevels, _edgeThreshold, _firstLevel, _scoreType, _patchSize, _fastThreshold, _useAgast ? 1 : 0,
	                    _fastAgastType, _do_dBrief ? 1 : 0, _learnMasks ? 1 : 0, _descSize} {}
	~mdBRIEFextractorOct() { if (ex_) mcs_extractor_destroy(ex_); }

	// operator()(image, mask, keypoints, camModel, descriptors, descriptorMasks)  (src/mdBRIEFextractorOct.cpp:1244-1337)
	void operator()(const Mat8u& image, const Mat8u& mask, std::vector<KeyPoint>& keypoints, cCamModelGeneral_& camModel, Mat8u& descriptors,
	                Mat8u& descriptorMasks) {
		extract(image, mask, keypoints, &camModel.ocam, descriptors, descriptorMasks);
	}
	// the same with an optional camera model (ORB mode reads none: ORBextractor below)
	void extract(const Mat8u& image, const Mat8u& mask, std::vector<KeyPoint>& keypoints, const mcs_ocam* ocam, Mat8u& descriptors, Mat8u& descriptorMasks) {
		if (image.empty()) return;   // :1252-1253
		ensure(image.cols, image.rows, 1);
		std::vector<mcs_keypoint> kps(cap_);
		std::vector<uint8_t> d((size_t)cap_ * p_.descSize), m((size_t)cap_ * p_.descSize);
		int32_t n = 0;
		mcs_throw(mcs_extract_batch(ex_, 1, image.data, 0, image.step, mask.empty() ? nullptr : mask.data, 0, mask.step, ocam,
		                            MCS_MEM_HOST, &n, kps.data(), d.data(), m.data(), nullptr));
		keypoints.resize(n);
		if (n) std::memcpy(keypoints.data(), kps.data(), (size_t)n * sizeof(KeyPoint));
		if (n == 0) { descriptors.release(); descriptorMasks.release(); return; }   // :1270-1274
		descriptors.create(n, p_.descSize);
		descriptorMasks.create(n, p_.descSize);
		std::memcpy(descriptors.data, d.data(), (size_t)n * p_.descSize);
		std::memcpy(descriptorMasks.data, m.data(), (size_t)n * p_.descSize);
	}

	// All cameras of a rig in one device batch (the GPU analogue of `#pragma omp parallel for num_threads(nrCams)`,
	// src/cMultiFrame.cpp:128); also returns the rays of src/cMultiFrame.cpp:146-152.
	void extractRig(const std::vector<const uint8_t*>& images, int width, int height, int stride, const std::vector<const uint8_t*>& masks,
	                const std::vector<mcs_ocam>& cams, std::vector<std::vector<KeyPoint>>& keys, std::vector<Mat8u>& desc, std::vector<Mat8u>& dmask,
	                std::vector<std::vector<Vec3d>>& rays) {
		const int n = (int)images.size();
		ensure(width, height, n);
		std::vector<uint8_t> img((size_t)n * stride * height), msk;
		for (int i = 0; i < n; ++i) std::memcpy(img.data() + (size_t)i * stride * height, images[i], (size_t)stride * height);
		if (!masks.empty()) {
			msk.resize(img.size());
			for (int i = 0; i < n; ++i) std::memcpy(msk.data() + (size_t)i * stride * height, masks[i], (size_t)stride * height);
		}
		std::vector<int32_t> nkp(n);
		std::vector<mcs_keypoint> kps((size_t)n * cap_);
		std::vector<uint8_t> d((size_t)n * cap_ * p_.descSize), m(d.size());
		std::vector<double> r((size_t)n * cap_ * 3);
		mcs_throw(mcs_extract_batch(ex_, n, img.data(), (size_t)stride * height, stride, msk.empty() ? nullptr : msk.data(), (size_t)stride * height,
		                            stride, cams.data(), MCS_MEM_HOST, nkp.data(), kps.data(), d.data(), m.data(), r.data()));
		keys.assign(n, {}); desc.assign(n, {}); dmask.assign(n, {}); rays.assign(n, {});
		for (int i = 0; i < n; ++i) {
			const int k = nkp[i];
			keys[i].resize(k); rays[i].resize(k);
			if (!k) continue;
			std::memcpy(keys[i].data(), kps.data() + (size_t)i * cap_, (size_t)k * sizeof(KeyPoint));
			std::memcpy(rays[i].data(), r.data() + (size_t)i * cap_ * 3, (size_t)k * sizeof(Vec3d));
			desc[i].create(k, p_.descSize); dmask[i].create(k, p_.descSize);
			std::memcpy(desc[i].data, d.data() + (size_t)i * cap_ * p_.descSize, (size_t)k * p_.descSize);
			std::memcpy(dmask[i].data, m.data() + (size_t)i * cap_ * p_.descSize, (size_t)k * p_.descSize);
		}
	}

	int GetLevels() { return p_.nlevels; }
	double GetScaleFactor() { return (double)p_.scaleFactor; }   // member is the double of the FLOAT ctor argument
	bool GetMasksLearned() { return p_.learnMasks != 0; }
	int GetDescriptorSize() { return p_.descSize; }

private:
	void ensure(int w, int h, int batch) {
		if (ex_ && w == w_ && h == h_ && batch <= batch_) return;
		if (ex_) mcs_extractor_destroy(ex_);
		ex_ = nullptr;
		mcs_throw(mcs_extractor_create(ctx_.h, &p_, w, h, batch, &ex_));
		mcs_throw(mcs_extractor_kp_capacity(ex_, &cap_));
		w_ = w; h_ = h; batch_ = batch;
	}
	Context& ctx_;
	mcs_extractor_params p_;
	mcs_extractor* ex_ = nullptr;
	int w_ = 0, h_ = 0, batch_ = 0, cap_ = 0;
};

// ---------------------------------------------------------------------------------------------- settings / calibration files
// The flat `key: value` subset of OpenCV FileStorage YAML the reference's Examples use (`%YAML:1.0` header, `#` comments).
inline std::map<std::string, std::string> ReadSettings(const std::string& path) {
	std::ifstream f(path);
	if (!f) throw std::runtime_error("cannot open " + path);
	std::map<std::string, std::string> out;
	std::string line;
	while (std::getline(f, line)) {
		const size_t h = line.find('#');
		if (h != std::string::npos) line.erase(h);
		const size_t c = line.find(':');
		if (line.empty() || line[0] == '%' || c == std::string::npos) continue;
		auto trim = [](std::string v) { const size_t a = v.find_first_not_of(" \t\r\""), b = v.find_last_not_of(" \t\r\""); return a == std::string::npos ? std::string() : v.substr(a, b - a + 1); };
		const std::string k = trim(line.substr(0, c)), v = trim(line.substr(c + 1));
		if (!k.empty() && !v.empty()) out[k] = v;
	}
	return out;
}
inline double SettingD(const std::map<std::string, std::string>& s, const std::string& k) {
	auto it = s.find(k);
	if (it == s.end()) throw std::runtime_error("missing setting " + k);
	return std::strtod(it->second.c_str(), nullptr);
}
inline int SettingI(const std::map<std::string, std::string>& s, const std::string& k) { return (int)SettingD(s, k); }

// CreateMirrorMask (src/cam_model_omni.cpp:181-220), level 0: float arithmetic, the principal-point names swapped like the reference
inline void CreateMirrorMask0(const mcs_ocam& cam, Mat8u& mask) {
	const int w = cam.width, h = cam.height;
	const float u0 = (float)cam.v0, v0 = (float)cam.u0;
	mask.create(h, w);
	for (int i = 0; i < h; ++i)
		for (int j = 0; j < w; ++j) {
			const float ans = std::sqrt((float)std::pow((double)(i - u0), 2) + (float)std::pow((double)(j - v0), 2));
			mask.data[(size_t)i * w + j] = ans < (u0 + 22.0f) ? 255 : 0;
		}
}

using Matx44d = std::array<double, 16>;   // row-major
inline Matx44d MatMul(const Matx44d& A, const Matx44d& B) {   // cv::Matx product: s = 0; s += a(i,k) * b(k,j)
	Matx44d C{};
	for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { double s = 0; for (int k = 0; k < 4; ++k) s += A[4 * i + k] * B[4 * k + j]; C[4 * i + j] = s; }
	return C;
}
inline Matx44d InvMat(const Matx44d& M) {   // cConverter::invMat (src/cConverter.cpp:31-44): rigid inverse, t = -(R^T) t
	Matx44d o{};
	for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) o[4 * i + j] = M[4 * j + i];
	for (int i = 0; i < 3; ++i) { double s = 0; for (int k = 0; k < 3; ++k) s += -o[4 * i + k] * M[4 * k + 3]; o[4 * i + 3] = s; }
	o[15] = 1.0;
	return o;
}
inline Matx44d Cayley2Hom(const double c[6]) {   // include/misc.h:132-160, 211-224
	const double c1 = c[0], c2 = c[1], c3 = c[2], a = c1 * c1, b = c2 * c2, g = c3 * c3, sc = 1.0 / (1.0 + a + b + g);
	const double R[9] = {1 + a - b - g, 2 * (c1 * c2 - c3), 2 * (c1 * c3 + c2), 2 * (c1 * c2 + c3), 1 - a + b - g, 2 * (c2 * c3 - c1),
	                     2 * (c1 * c3 - c2), 2 * (c2 * c3 + c1), 1 - a - b + g};
	Matx44d M{};
	for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) M[4 * i + j] = sc * R[3 * i + j]; M[4 * i + 3] = c[3 + i]; }
	M[15] = 1.0;
	return M;
}

// ORBextractor (include/cORBextractor.h:48-67; the reference declares the class and never compiles an implementation): the extractor in ORB mode behind the
// five-argument constructor and the four-argument operator() — no camera model, no descriptor masks.  scaleFactor is a double in this header (a float in
// mdBRIEFextractorOct's): it is narrowed to the float the extraction tables are built from, and GetScaleFactor() returns what was passed.
class ORBextractor {
public:
	enum { HARRIS_SCORE = 0, FAST_SCORE = 1 };
	ORBextractor(Context& ctx, int nfeatures = 1000, double scaleFactor = 1.2, int nlevels = 8, int scoreType = FAST_SCORE, int fastTh = 20)
	    : impl_(ctx, nfeatures, (float)scaleFactor, nlevels, 25, 0, scoreType, 32, fastTh, false, 2, false, false, 32), nlevels_(nlevels), scaleFactor_(scaleFactor) {}
	// operator()(image, mask, keypoints, descriptors)   (include/cORBextractor.h:61-63)
	void operator()(const Mat8u& image, const Mat8u& mask, std::vector<KeyPoint>& keypoints, Mat8u& descriptors) {
		Mat8u unusedMasks;
		impl_.extract(image, mask, keypoints, nullptr, descriptors, unusedMasks);   // ORB mode reads no camera model
	}
	int GetLevels() { return nlevels_; }
	double GetScaleFactor() { return scaleFactor_; }

private:
	mdBRIEFextractorOct impl_;
	int nlevels_;
	double scaleFactor_;
};

// cMultiCamSys_ (include/cam_system_omni.h): calibrations + poses; the projection of many points runs on the GPU in one call
class cMultiCamSys_ {
public:
	std::vector<cCamModelGeneral_> camModels;
	std::vector<Matx44d> M_c, MtMc, MtMc_inv;
	Matx44d M_t{};
	std::vector<std::array<double, 6>> M_c_min;   // Get_M_c_min(c): the calibration's Cayley parameters and translations (LoadMCS fills them)
	std::array<double, 6> M_t_min{};              // GetPoseMin(): what Set_M_t_from_min was given last
	int GetNrCams() const { return (int)camModels.size(); }
	// src/cam_system_omni.cpp:170-183.  MtMc_ / MtMc_inv_ (nrCams x 16 doubles each): the products as a device call built them, instead of building them here.
	void Set_M_t_from_min(const std::array<double, 6>& M_t_minRep, const double* MtMc_ = nullptr, const double* MtMc_inv_ = nullptr) {
		M_t_min = M_t_minRep;
		M_t = Cayley2Hom(M_t_min.data());
		MtMc.resize(M_c.size()); MtMc_inv.resize(M_c.size());
		for (size_t c = 0; c < M_c.size(); ++c) {
			if (MtMc_ && MtMc_inv_) { std::memcpy(MtMc[c].data(), MtMc_ + 16 * c, 128); std::memcpy(MtMc_inv[c].data(), MtMc_inv_ + 16 * c, 128); }
			else { MtMc[c] = MatMul(M_t, M_c[c]); MtMc_inv[c] = InvMat(MtMc[c]); }
		}
	}
	cCamModelGeneral_& GetCamModelObj(int c) { return camModels[c]; }
	void Set_M_t(const Matx44d& M) {   // src/cam_system_omni.cpp:184-198
		M_t = M;
		MtMc.resize(M_c.size()); MtMc_inv.resize(M_c.size());
		for (size_t c = 0; c < M_c.size(); ++c) { MtMc[c] = MatMul(M_t, M_c[c]); MtMc_inv[c] = InvMat(MtMc[c]); }
	}
	// WorldToCamHom_fast + isPointInMirrorMask(u, v, 0) for n points (point i into camera cam[i]): uv = 2 doubles per point,
	// flags bit0 = inside the mirror mask, bit1 = behind the camera (src/cam_system_omni.cpp:92-133, src/cam_model_omni.cpp:163-178)
	void WorldToCamHom_fast(Context& ctx, const double* pts3, const int32_t* cam, int n, double* uv, uint8_t* flags) {
		std::vector<mcs_ocam> oc;
		std::vector<const uint8_t*> masks;
		bool any = false;
		for (auto& m : camModels) { oc.push_back(m.ocam); masks.push_back(m.mirrorMask0.empty() ? nullptr : m.mirrorMask0.data); any = any || !m.mirrorMask0.empty(); }
		std::vector<double> M((size_t)GetNrCams() * 16);
		for (int c = 0; c < GetNrCams(); ++c) std::memcpy(&M[16 * (size_t)c], MtMc_inv[c].data(), 128);
		mcs_throw(mcs_world_to_cam(ctx.h, M.data(), oc.data(), GetNrCams(), any ? masks.data() : nullptr, pts3, cam, n, MCS_MEM_HOST, uv, flags));
	}
};

// cSystem::LoadMCS (src/cSystem.cpp:125-180): MultiCamSys_Calibration.yaml + InteriorOrientationFisheye<c>.yaml, M_t = identity
inline void LoadMCS(const std::string& path2calibrations, cMultiCamSys_& camSystem) {
	const auto mcs = ReadSettings(path2calibrations + "/MultiCamSys_Calibration.yaml");
	const int nrCams = SettingI(mcs, "CameraSystem.nrCams");
	camSystem.camModels.assign(nrCams, {});
	camSystem.M_c.assign(nrCams, {});
	camSystem.M_c_min.assign(nrCams, {});
	for (int c = 0; c < nrCams; ++c) {
		double cay[6];
		for (int p = 1; p < 7; ++p) cay[p - 1] = SettingD(mcs, "CameraSystem.cam" + std::to_string(c + 1) + "_" + std::to_string(p));
		camSystem.M_c[c] = Cayley2Hom(cay);
		std::copy(cay, cay + 6, camSystem.M_c_min[c].begin());
		const auto fs = ReadSettings(path2calibrations + "/InteriorOrientationFisheye" + std::to_string(c) + ".yaml");
		mcs_ocam& o = camSystem.camModels[c].ocam;
		std::memset(&o, 0, sizeof(o));
		const int nrpol = SettingI(fs, "Camera.nrpol"), nrinvpol = SettingI(fs, "Camera.nrinvpol");
		if (nrpol > MCS_MAX_POLY || nrinvpol > MCS_MAX_POLY) throw std::runtime_error("polynomial degree above MCS_MAX_POLY");
		for (int i = 0; i < nrpol; ++i) o.p[i] = SettingD(fs, "Camera.a" + std::to_string(i));
		for (int i = 0; i < nrinvpol; ++i) o.invP[i] = SettingD(fs, "Camera.pol" + std::to_string(i));
		o.p_deg = nrpol > 5 ? nrpol : 5; o.invP_deg = nrinvpol > 12 ? nrinvpol : 12;   // cv::Mat::zeros(5,1) / zeros(12,1) in the reference
		o.width = SettingI(fs, "Camera.Iw"); o.height = SettingI(fs, "Camera.Ih");
		o.c = SettingD(fs, "Camera.c"); o.d = SettingD(fs, "Camera.d"); o.e = SettingD(fs, "Camera.e"); o.u0 = SettingD(fs, "Camera.u0"); o.v0 = SettingD(fs, "Camera.v0");
		if (SettingI(fs, "Camera.mirrorMask") == 1) CreateMirrorMask0(o, camSystem.camModels[c].mirrorMask0);
		else { camSystem.camModels[c].mirrorMask0.create(o.height, o.width); std::memset(camSystem.camModels[c].mirrorMask0.data, 1, (size_t)o.width * o.height); }
	}
	Matx44d I{}; I[0] = I[5] = I[10] = I[15] = 1.0;
	camSystem.Set_M_t(I);
}

// ORBVocabulary (include/cORBVocabulary.h = DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>) as far as cMultiFrame::ComputeBoW uses it
class cORBVocabulary {
public:
	using BowVector = std::map<unsigned, double>;                       // DBoW2::BowVector
	using FeatureVector = std::map<unsigned, std::vector<unsigned>>;    // DBoW2::FeatureVector
	cORBVocabulary(Context& ctx) : ctx_(ctx) {}
	~cORBVocabulary() { if (h_) mcs_vocabulary_destroy(h_); }
	cORBVocabulary(const cORBVocabulary&) = delete;
	cORBVocabulary& operator=(const cORBVocabulary&) = delete;
	// TemplatedVocabulary::load from the OpenCV-YAML vocabulary file (ThirdParty/DBoW2/DBoW2/TemplatedVocabulary.h:1573-1622)
	void load(const std::string& path) {
		std::ifstream f(path);
		if (!f) throw std::runtime_error("cannot open " + path);
		std::stringstream ss; ss << f.rdbuf();
		const std::string t = ss.str();
		auto intAfter = [&](const std::string& key, size_t from, size_t& pos) { pos = t.find(key, from); return pos == std::string::npos ? -1L : std::strtol(t.c_str() + pos + key.size(), nullptr, 10); };
		size_t p;
		m_k = (int)intAfter(" k:", 0, p); m_L = (int)intAfter(" L:", 0, p);   // (" L:" — the header line "%YAML:1.0" also contains "L:")
		if (intAfter("scoringType:", 0, p) != 0 || intAfter("weightingType:", 0, p) != 0) throw std::runtime_error("only TF_IDF / L1 vocabularies are mirrored");
		struct N { int id, parent; double w; uint8_t d[32]; };
		std::vector<N> nodes;
		size_t pos = t.find("nodes:");
		const size_t wordsAt = t.find("words:");
		while (true) {
			size_t q;
			N n{};
			n.id = (int)intAfter("nodeId:", pos, q);
			if (q == std::string::npos || q > wordsAt) break;
			n.parent = (int)intAfter("parentId:", q, p);
			size_t wq = t.find("weight:", q);
			n.w = std::strtod(t.c_str() + wq + 7, nullptr);
			size_t dq = t.find('"', wq) + 1;
			const char* c = t.c_str() + dq;
			for (int i = 0; i < 32; ++i) { char* e; n.d[i] = (uint8_t)std::strtol(c, &e, 10); c = e; }
			nodes.push_back(n);
			pos = t.find('}', dq);
		}
		const int nn = (int)nodes.size() + 1;
		nodeDesc.assign((size_t)nn * 32, 0); weight.assign(nn, 0.0); wordId.assign(nn, -1);
		std::vector<std::vector<int>> ch(nn);
		for (auto& n : nodes) { std::memcpy(&nodeDesc[(size_t)n.id * 32], n.d, 32); weight[n.id] = n.w; ch[n.parent].push_back(n.id); }
		childOff.assign(nn + 1, 0); childIdx.clear();
		for (int i = 0; i < nn; ++i) { childOff[i + 1] = childOff[i] + (int)ch[i].size(); childIdx.insert(childIdx.end(), ch[i].begin(), ch[i].end()); }
		pos = wordsAt;
		while (true) {
			size_t q;
			const long wid = intAfter("wordId:", pos, q);
			if (q == std::string::npos) break;
			wordId[intAfter("nodeId:", q, p)] = (int)wid;
			pos = q + 7;
		}
		if (h_) { mcs_vocabulary_destroy(h_); h_ = nullptr; }
		mcs_throw(mcs_vocabulary_create(ctx_.h, nn, nodeDesc.data(), childOff.data(), childIdx.data(), m_L, &h_));
		mcs_throw(mcs_vocabulary_set_words(h_, wordId.data(), weight.data()));
		m_words = 0;
		for (int32_t w : wordId) m_words = w + 1 > m_words ? w + 1 : m_words;
	}
	unsigned size() const { return (unsigned)m_words; }   // TemplatedVocabulary::size(): number of words
	// score(a, b) = L1Scoring::score (ThirdParty/DBoW2/DBoW2/ScoringObject.cpp:23-66): one pair, shared words in ascending id order, vi from a.
	// The loop closer's many pairs against stored keyframes go through cMultiKeyFrameDatabase::score on the device.
	double score(const BowVector& a, const BowVector& b) const {
		double s = 0;
		auto i = a.begin(), j = b.begin();
		while (i != a.end() && j != b.end()) {
			if (i->first == j->first) { const double vi = i->second, wi = j->second; s += std::fabs(vi - wi) - std::fabs(vi) - std::fabs(wi); ++i; ++j; }
			else if (i->first < j->first) i = a.lower_bound(j->first);
			else j = b.lower_bound(i->first);
		}
		return -s / 2.0;
	}
	// the BowVector of transform() built on the device from the leaf nodes (mcs_bow_vector); v is identical to transform()'s
	void transformBow(const uint8_t* descriptors, int n, int stride, BowVector& v, int levelsup = 4) {
		v.clear();
		if (!h_ || n <= 0) return;
		std::vector<int32_t> leaf(n), nid(n), w(n);
		std::vector<double> val(n);
		int32_t nw = 0;
		mcs_throw(mcs_bow_transform(h_, descriptors, n, stride, levelsup, MCS_MEM_HOST, leaf.data(), nid.data()));
		mcs_throw(mcs_bow_vector(h_, leaf.data(), n, MCS_MEM_HOST, w.data(), val.data(), &nw));
		for (int i = 0; i < nw; ++i) v.emplace_hint(v.end(), (unsigned)w[i], val[i]);
	}
	mcs_vocabulary* handle() const { return h_; }
	// transform(features, v, fv, levelsup) (:1127-1205, TF_IDF weighting, L1 scoring): descriptors = n rows of `stride` >= 32 bytes
	void transform(const uint8_t* descriptors, int n, int stride, BowVector& v, FeatureVector& fv, int levelsup) {
		v.clear(); fv.clear();
		if (!h_ || n <= 0) return;
		std::vector<int32_t> leaf(n), nid(n);
		mcs_throw(mcs_bow_transform(h_, descriptors, n, stride, levelsup, MCS_MEM_HOST, leaf.data(), nid.data()));
		for (int i = 0; i < n; ++i) {
			const double w = weight[leaf[i]];
			if (w > 0) { v[(unsigned)wordId[leaf[i]]] += w; fv[(unsigned)nid[i]].push_back((unsigned)i); }
		}
		double norm = 0.0;
		for (auto& e : v) norm += std::fabs(e.second);
		if (norm > 0.0) for (auto& e : v) e.second /= norm;
	}
	int m_k = 0, m_L = 0, m_words = 0;
	std::vector<uint8_t> nodeDesc; std::vector<int32_t> childOff, childIdx, wordId; std::vector<double> weight;
private:
	Context& ctx_;
	mcs_vocabulary* h_ = nullptr;
};

// cMapPoint::ComputeDistinctiveDescriptors (src/cMapPoint.cpp:294-382) for a batch: offsets = CSR rows of the observed descriptors
inline void ComputeDistinctiveDescriptors(Context& ctx, const uint8_t* desc, const uint8_t* mask, int stride, int dim, const std::vector<int32_t>& offsets,
                                          std::vector<int32_t>& bestIdx) {
	const int np = (int)offsets.size() - 1;
	bestIdx.assign(np > 0 ? np : 0, -1);
	if (np > 0) mcs_throw(mcs_distinctive_descriptors(ctx.h, desc, mask, stride, dim, offsets.data(), np, MCS_MEM_HOST, bestIdx.data()));
}

// flat view of a (multi-)keyframe / frame as the brute-force searches see it: all cameras concatenated in mvKeys order
struct FeatureSetView {
	const uint8_t* descriptors = nullptr;   // n x dim
	const uint8_t* masks = nullptr;         // n x dim or nullptr
	std::vector<uint8_t> flag;              // meaning depends on the search (see cORBmatcher)
	std::vector<int32_t> cam;               // keypoint_to_cam
	const double* rays = nullptr;           // n x 3
	int n = 0;
};

class cORBmatcher {
public:
	cORBmatcher(Context& ctx, double nnratio = 0.6, bool checkOri = true, int featDim = 32, bool havingMasks_ = false, int K = 32)
	    : ctx_(ctx), mfNNratio(nnratio), mbFeatDim(featDim), havingMasks(havingMasks_), K_(K) {
		mbCheckOrientation = checkOri;   // the searches below return unfiltered matches; RotationConsistency() is the separate pass of the reference's flag
	}
	// mbCheckOrientation pass (ComputeThreeMaxima, :2394-2436) on a match array (slot -> partner or -1); variant / swapped per search are listed at
	// mcs_rotation_consistency in mcs_c.h.  Returns the number of matches removed; a no-op unless the matcher was built with checkOri = true.
	int RotationConsistency(int variant, const KeyPoint* slotKeys, const KeyPoint* partnerKeys, int nPartner, std::vector<int>& match, bool swapped,
	                        const std::vector<int>* accepted = nullptr) {
		if (!mbCheckOrientation || match.empty() || nPartner <= 0) return 0;
		int32_t removed = 0;
		mcs_throw(mcs_rotation_consistency(ctx_.h, variant, &slotKeys[0].angle, (int)sizeof(KeyPoint), &partnerKeys[0].angle, (int)sizeof(KeyPoint),
		                                   accepted ? accepted->data() : nullptr, match.data(), (int)match.size(), nPartner, swapped ? 1 : 0, MCS_MEM_HOST, &removed));
		return removed;
	}
	// SearchByBoW(pKF1, pKF2, vpMatches12): flag = "has a good map point".  match12[i] = index in kf2 or -1.  (:885-966)
	int SearchByBoW(const FeatureSetView& kf1, const FeatureSetView& kf2, std::vector<int>& match12) {
		return run(0, kf1, kf2, nullptr, 0, match12, kf1.n);
	}
	// SearchByBoW(pKF, F, vpMapPointMatches) without the vocabulary restriction: matchF[j] = keyframe feature or -1.  (:179-323)
	int SearchByBoWFrame(const FeatureSetView& kf, const FeatureSetView& frame, std::vector<int>& matchF) {
		return run(1, kf, frame, nullptr, 0, matchF, frame.n);
	}
	// SearchForTriangulationRaw: flag = "has NO map point", cam + rays required, E = nrCams*nrCams 3x3 row-major.  (:968-1155)
	int SearchForTriangulationRaw(const FeatureSetView& kf1, const FeatureSetView& kf2, const double* E, int nrCams,
	                              std::vector<std::pair<size_t, size_t>>& vMatchedPairs) {
		std::vector<int> m12;
		const int n = run(2, kf1, kf2, E, nrCams, m12, kf1.n);
		vMatchedPairs.clear();
		for (size_t i = 0; i < m12.size(); ++i) if (m12[i] >= 0) vMatchedPairs.emplace_back(i, (size_t)m12[i]);
		return n;
	}

	// ---- grid-window searches (src/cORBmatcher.cpp:326-726, 1990-2118).  A FrameGridView is the flat cMultiFrame the windows are opened in.
	struct FrameGridView {
		const KeyPoint* mvKeys = nullptr; const uint8_t* descriptors = nullptr; const uint8_t* masks = nullptr;
		std::vector<int32_t> keypoint_to_cam; std::vector<uint8_t> hasMapPoint;   // hasMapPoint[i] = mvpMapPoints[i] != NULL (updated by the searches)
		std::vector<int32_t> width, height; std::vector<double> mvScaleFactors; int n = 0;
		mcs_frame_view view(int dim, bool havingMasks, uint8_t* assigned) const {
			return mcs_frame_view{reinterpret_cast<const mcs_keypoint*>(mvKeys), descriptors, havingMasks ? masks : nullptr, keypoint_to_cam.data(), assigned, n, dim,
			                      (int32_t)width.size(), width.data(), height.data(), mvScaleFactors.data(), (int32_t)mvScaleFactors.size()};
		}
	};
	// WindowSearch(F1, F2, windowSize, vpMapPointMatches2, minScaleLevel, maxScaleLevel): good1[i1] = map point non-NULL && !isBad();
	// vnMatches21[i2] = i1 or -1.  (:326-473)
	int WindowSearch(const FrameGridView& F1, const std::vector<uint8_t>& good1, FrameGridView& F2, int windowSize, std::vector<int>& vnMatches21,
	                 int minScaleLevel = 0, int maxScaleLevel = INT32_MAX) {
		Probes p;
		for (int i1 = 0; i1 < F1.n; ++i1) {
			const int lvl = F1.mvKeys[i1].octave;
			if (!good1[i1] || (minScaleLevel > 0 && lvl < minScaleLevel) || (maxScaleLevel < INT32_MAX && lvl > maxScaleLevel)) continue;
			p.add(F1.mvKeys[i1].ptx, F1.mvKeys[i1].pty, windowSize, -1, -1, F1.keypoint_to_cam[i1], i1);
		}
		std::vector<uint8_t> none(F2.n > 0 ? F2.n : 1, 0);   // vpMapPointMatches2 starts all-NULL
		std::swap(none, F2.hasMapPoint);
		std::vector<int> m;
		const int nm = window(MCS_WINDOW_RATIO, p, F1, F2, m);
		std::swap(none, F2.hasMapPoint);
		vnMatches21.assign(F2.n, -1);
		for (size_t k = 0; k < m.size(); ++k) if (m[k] >= 0) vnMatches21[m[k]] = p.src[k];
		return nm;
	}
	// SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize): vbPrevMatched = 2 doubles per F1 feature, updated.  (:579-726)
	int SearchForInitialization(const FrameGridView& F1, FrameGridView& F2, std::vector<double>& vbPrevMatched, std::vector<int>& vnMatches12,
	                            int windowSize = 10) {
		Probes p;
		for (int i1 = 0; i1 < F1.n; ++i1)
			p.add(vbPrevMatched[2 * i1], vbPrevMatched[2 * i1 + 1], windowSize, F1.mvKeys[i1].octave, F1.mvKeys[i1].octave, F1.keypoint_to_cam[i1], i1);
		const int nm = window(MCS_WINDOW_INITIALIZE, p, F1, F2, vnMatches12);
		vnMatches12.resize(F1.n);
		for (int i1 = 0; i1 < F1.n; ++i1)
			if (vnMatches12[i1] >= 0) { vbPrevMatched[2 * i1] = F2.mvKeys[vnMatches12[i1]].ptx; vbPrevMatched[2 * i1 + 1] = F2.mvKeys[vnMatches12[i1]].pty; }
		return nm;
	}
	// SearchByProjection(CurrentFrame, LastFrame, th): search1[i] = map point good && !mvbOutlier[i] && projection inside the mirror mask;
	// uv = the projections (mcs_world_to_cam).  matchCur[i2] = index in LastFrame or -1; CurrentFrame.hasMapPoint is updated.  (:1990-2118)
	int SearchByProjection(FrameGridView& CurrentFrame, const FrameGridView& LastFrame, const std::vector<uint8_t>& search1, const double* uv, double th,
	                       std::vector<int>& matchCur) {
		Probes p;
		for (int i = 0; i < LastFrame.n; ++i) {
			if (!search1[i]) continue;
			const int o = LastFrame.mvKeys[i].octave;
			p.add(uv[2 * i], uv[2 * i + 1], th * CurrentFrame.mvScaleFactors[o], o - 1, o + 1, LastFrame.keypoint_to_cam[i], i);
		}
		std::vector<int> m;
		const int nm = window(MCS_WINDOW_BEST, p, LastFrame, CurrentFrame, m);
		matchCur.assign(CurrentFrame.n, -1);
		for (size_t k = 0; k < m.size(); ++k) if (m[k] >= 0) matchCur[m[k]] = p.src[k];
		return nm;
	}

	// SearchByProjection(F, vpMapPoints, th) (:67-166): one projection per (map point, camera) with mbTrackInView, in the reference's order;
	// match[p] = frame feature or -1; F.hasMapPoint is updated.
	struct Projections { std::vector<double> x, y, viewCos; std::vector<int32_t> level, cam; const uint8_t* desc = nullptr; const uint8_t* mask = nullptr; };
	int SearchByProjection(FrameGridView& F, const Projections& mp, double th, std::vector<int>& match) {
		const int n = (int)mp.x.size();
		mcs_projection_set ps{mp.x.data(), mp.y.data(), mp.viewCos.data(), mp.level.data(), mp.cam.data(), mp.desc, havingMasks ? mp.mask : nullptr, n, mbFeatDim};
		const mcs_frame_view fv = F.view(mbFeatDim, havingMasks, F.hasMapPoint.data());
		match.assign(n > 0 ? n : 1, -1);
		int32_t nm = 0;
		mcs_throw(mcs_search_by_projection(ctx_.h, &ps, &fv, th, mfNNratio, mbFeatDim, MCS_MEM_HOST, match.data(), &nm));
		match.resize(n);
		return nm;
	}
	// The search loop of Fuse / SearchBySim3 / SearchForTriangulationBetweenCameras (skipTaken = false) and of the relocalisation
	// SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (skipTaken = true): closest feature per window, accepted if <= maxDist.
	struct Windows { std::vector<double> x, y, r; std::vector<int32_t> lo, hi, cam; const uint8_t* desc = nullptr; const uint8_t* mask = nullptr; };
	int BestInWindows(FrameGridView& F, const Windows& w, int maxDist, bool skipTaken, std::vector<int>& match, std::vector<int>& dist) {
		const int n = (int)w.x.size();
		mcs_window_probes pr{w.x.data(), w.y.data(), w.r.data(), w.lo.data(), w.hi.data(), w.cam.data(), w.desc, havingMasks ? w.mask : nullptr, n, mbFeatDim};
		const mcs_frame_view fv = F.view(mbFeatDim, havingMasks, skipTaken ? F.hasMapPoint.data() : nullptr);
		match.assign(n > 0 ? n : 1, -1); dist.assign(n > 0 ? n : 1, 0);
		int32_t nm = 0;
		mcs_throw(mcs_window_best(ctx_.h, &pr, &fv, maxDist, skipTaken ? 1 : 0, mbFeatDim, MCS_MEM_HOST, match.data(), dist.data(), &nm));
		match.resize(n); dist.resize(n);
		return nm;
	}
	// SearchByBoW(pKF, F, ...) WITH the vocabulary (:179-323): kf rows must be given in FeatureVector order (node ascending, index ascending),
	// `cam` of both views carries the FeatureVector node id (frame features of stopped words: flag 0).  matchF[j] = kf row or -1.
	int SearchByBoWFrameVocabulary(const FeatureSetView& kfInNodeOrder, const FeatureSetView& frame, std::vector<int>& matchF) {
		mcs_desc_set q{kfInNodeOrder.descriptors, havingMasks ? kfInNodeOrder.masks : nullptr, kfInNodeOrder.flag.data(), kfInNodeOrder.cam.data(), kfInNodeOrder.n, mbFeatDim};
		mcs_desc_set t{frame.descriptors, havingMasks ? frame.masks : nullptr, frame.flag.empty() ? nullptr : frame.flag.data(), frame.cam.data(), frame.n, mbFeatDim};
		matchF.assign(frame.n > 0 ? frame.n : 1, -1);
		int32_t nm = 0, fb = 0;
		mcs_throw(mcs_search_kf_f(ctx_.h, 1, &q, 0, &t, 0, mbFeatDim, mfNNratio, K_, MCS_MEM_HOST, matchF.data(), &nm, &fb));
		matchF.resize(frame.n);
		return nm;
	}

private:
	struct Probes {
		std::vector<double> x, y, r; std::vector<int32_t> lo, hi, cam, src;
		void add(double x_, double y_, double r_, int lo_, int hi_, int cam_, int src_) {
			x.push_back(x_); y.push_back(y_); r.push_back(r_); lo.push_back(lo_); hi.push_back(hi_); cam.push_back(cam_); src.push_back(src_);
		}
	};
	int window(mcs_window_rule rule, const Probes& p, const FrameGridView& from, FrameGridView& in, std::vector<int>& match) {
		const int n = (int)p.x.size();
		std::vector<uint8_t> d((size_t)(n > 0 ? n : 1) * mbFeatDim), m(havingMasks ? d.size() : 0);
		for (int k = 0; k < n; ++k) {
			std::memcpy(&d[(size_t)k * mbFeatDim], from.descriptors + (size_t)p.src[k] * mbFeatDim, mbFeatDim);
			if (havingMasks) std::memcpy(&m[(size_t)k * mbFeatDim], from.masks + (size_t)p.src[k] * mbFeatDim, mbFeatDim);
		}
		mcs_window_probes pr{p.x.data(), p.y.data(), p.r.data(), p.lo.data(), p.hi.data(), p.cam.data(), d.data(), havingMasks ? m.data() : nullptr, n, mbFeatDim};
		const mcs_frame_view fv = in.view(mbFeatDim, havingMasks, rule == MCS_WINDOW_INITIALIZE ? nullptr : in.hasMapPoint.data());
		match.assign(n > 0 ? n : 1, -1);
		int32_t nm = 0;
		mcs_throw(mcs_window_match(ctx_.h, &pr, &fv, rule, mfNNratio, mbFeatDim, MCS_MEM_HOST, match.data(), &nm));
		match.resize(n);
		return nm;
	}
	int run(int mode, const FeatureSetView& a, const FeatureSetView& b, const double* E, int nrCams, std::vector<int>& out, int outN) {
		mcs_desc_set q{a.descriptors, havingMasks ? a.masks : nullptr, a.flag.empty() ? nullptr : a.flag.data(), mode == 2 ? a.cam.data() : nullptr, a.n, mbFeatDim};
		mcs_desc_set t{b.descriptors, havingMasks ? b.masks : nullptr, (mode == 1 || b.flag.empty()) ? nullptr : b.flag.data(), mode == 2 ? b.cam.data() : nullptr, b.n, mbFeatDim};
		out.assign(outN > 0 ? outN : 1, -1);
		int32_t nm = 0, fb = 0;
		int rc;
		if (mode == 0) rc = mcs_search_kf_kf(ctx_.h, 1, &q, 0, &t, 0, mbFeatDim, mfNNratio, K_, MCS_MEM_HOST, out.data(), &nm, &fb);
		else if (mode == 1) rc = mcs_search_kf_f(ctx_.h, 1, &q, 0, &t, 0, mbFeatDim, mfNNratio, K_, MCS_MEM_HOST, out.data(), &nm, &fb);
		else rc = mcs_search_triangulation(ctx_.h, 1, &q, 0, &t, 0, a.rays, b.rays, E, nrCams, mbFeatDim, K_, MCS_MEM_HOST, out.data(), &nm, &fb);
		mcs_throw(rc);
		out.resize(outN);
		return nm;
	}
	Context& ctx_;
	double mfNNratio;
	int mbFeatDim;
	bool havingMasks;
	int K_;
	bool mbCheckOrientation = false;
};

inline int DescriptorDistance64(Context& c, const uint64_t* descr_i, const uint64_t* descr_j, const int& dim) {
	int out = 0;
	mcs_throw(mcs_descriptor_distance(c.h, (const uint8_t*)descr_i, (const uint8_t*)descr_j, dim, &out));
	return out;
}
inline int DescriptorDistance64Masked(Context& c, const uint64_t* descr_i, const uint64_t* descr_j, const uint64_t* mask_i, const uint64_t* mask_j,
                                      const int& dim) {
	int out = 0;
	mcs_throw(mcs_descriptor_distance_masked(c.h, (const uint8_t*)descr_i, (const uint8_t*)descr_j, (const uint8_t*)mask_i, (const uint8_t*)mask_j, dim, &out));
	return out;
}

// cMultiKeyFrameDatabase (src/cMultiKeyFrameDatabase.cpp) over mcs_kfdb_*.  KF: the caller's keyframe / frame type with `mnId` and
// `mBowVec` (a std::map<word, value> as DBoW2::BowVector).  The covisibility the queries read (GetBestCovisibilityKeyFrames(10),
// src/cMultiKeyFrame.cpp:231-240) is handed over with SetCovisibility whenever it changes; the connected set of a loop query is an argument.
// Candidates come back as the KF pointers that were added or named as neighbours.
template <class KF>
class cMultiKeyFrameDatabase {
public:
	cMultiKeyFrameDatabase(Context& ctx, const cORBVocabulary& voc, int capacityHint = 0) { mcs_throw(mcs_kfdb_create(ctx.h, (int)voc.size(), capacityHint, &h_)); }
	cMultiKeyFrameDatabase(Context& ctx, int nWords, int capacityHint = 0) { mcs_throw(mcs_kfdb_create(ctx.h, nWords, capacityHint, &h_)); }
	~cMultiKeyFrameDatabase() { if (h_) mcs_kfdb_destroy(h_); }
	cMultiKeyFrameDatabase(const cMultiKeyFrameDatabase&) = delete;
	cMultiKeyFrameDatabase& operator=(const cMultiKeyFrameDatabase&) = delete;

	void add(KF* pKF) {   // :43-51
		std::vector<int32_t> off, w; std::vector<double> v; std::vector<int64_t> ids;
		csr(std::vector<KF*>{pKF}, ids, off, w, v);
		mcs_throw(mcs_kfdb_add(h_, 1, ids.data(), off.data(), w.data(), v.data(), MCS_MEM_HOST));
		obj_[(int64_t)pKF->mnId] = pKF;
	}
	void erase(KF* pKF) { const int64_t id = (int64_t)pKF->mnId; mcs_throw(mcs_kfdb_erase(h_, 1, &id)); }   // :53-73
	void clear() { mcs_throw(mcs_kfdb_clear(h_)); }                                                          // :75-79
	void SetCovisibility(KF* pKF, const std::vector<KF*>& orderedNeighbours) {
		const int64_t id = (int64_t)pKF->mnId;
		int64_t nb[10] = {0};
		const int32_t n = (int32_t)std::min<size_t>(orderedNeighbours.size(), 10);
		for (int k = 0; k < n; ++k) { nb[k] = (int64_t)orderedNeighbours[k]->mnId; obj_[nb[k]] = orderedNeighbours[k]; }
		obj_[id] = pKF;
		mcs_throw(mcs_kfdb_set_covisibility(h_, 1, &id, nb, &n));
	}
	template <class F>
	std::vector<KF*> DetectRelocalisationCandidates(F* pF) { return DetectRelocalisationCandidates(std::vector<F*>{pF})[0]; }   // :213-329
	template <class F>
	std::vector<std::vector<KF*>> DetectRelocalisationCandidates(const std::vector<F*>& frames) {   // the same queries one after another, in one call
		std::vector<int32_t> off, w; std::vector<double> v; std::vector<int64_t> ids;
		csr(frames, ids, off, w, v);
		return run(frames.size(), [&](int cap, int32_t* cnt, int64_t* out) {
			return mcs_kfdb_detect_relocalisation(h_, (int)frames.size(), ids.data(), off.data(), w.data(), v.data(), MCS_MEM_HOST, cap, cnt, out, nullptr); });
	}
	std::vector<KF*> DetectLoopCandidates(KF* pKF, double minScore, const std::set<KF*>& connected) {   // :82-210
		std::vector<int32_t> off, w; std::vector<double> v; std::vector<int64_t> ids, conn;
		csr(std::vector<KF*>{pKF}, ids, off, w, v);
		for (KF* k : connected) conn.push_back((int64_t)k->mnId);
		const int32_t coff[2] = {0, (int32_t)conn.size()};
		return run(1, [&](int cap, int32_t* cnt, int64_t* out) {
			return mcs_kfdb_detect_loop(h_, 1, ids.data(), off.data(), w.data(), v.data(), coff, conn.data(), &minScore, MCS_MEM_HOST, cap, cnt, out, nullptr); })[0];
	}
	// ORBVocabulary::score(bow, pKFi->mBowVec) for stored keyframes (src/cLoopClosing.cpp:132-151)
	template <class Bow>
	std::vector<double> score(const Bow& bow, const std::vector<KF*>& kfs) {
		std::vector<int32_t> w; std::vector<double> v, out(kfs.size()); std::vector<int64_t> ids;
		for (auto& e : bow) { w.push_back((int32_t)e.first); v.push_back(e.second); }
		for (KF* k : kfs) ids.push_back((int64_t)k->mnId);
		if (!kfs.empty()) mcs_throw(mcs_kfdb_score(h_, (int)w.size(), w.data(), v.data(), (int)ids.size(), ids.data(), MCS_MEM_HOST, out.data()));
		return out;
	}
	int size() const { int n = 0; mcs_throw(mcs_kfdb_size(h_, &n)); return n; }
	mcs_kfdb* handle() const { return h_; }

private:
	template <class T>
	static void csr(const std::vector<T*>& xs, std::vector<int64_t>& ids, std::vector<int32_t>& off, std::vector<int32_t>& w, std::vector<double>& v) {
		off.assign(1, 0);
		for (T* x : xs) {
			ids.push_back((int64_t)x->mnId);
			for (auto& e : x->mBowVec) { w.push_back((int32_t)e.first); v.push_back(e.second); }
			off.push_back((int32_t)w.size());
		}
	}
	template <class Call>
	std::vector<std::vector<KF*>> run(size_t nq, Call call) {
		const int cap = (int)obj_.size() + 1;   // a query returns each keyframe at most once
		std::vector<int32_t> cnt(nq);
		std::vector<int64_t> out(nq * (size_t)cap);
		mcs_throw(call(cap, cnt.data(), out.data()));
		std::vector<std::vector<KF*>> r(nq);
		for (size_t q = 0; q < nq; ++q)
			for (int i = 0; i < cnt[q]; ++i) r[q].push_back(obj_.at(out[q * cap + i]));
		return r;
	}
	mcs_kfdb* h_ = nullptr;
	std::map<int64_t, KF*> obj_;
};


// cSim3Solver (src/cSim3Solver.cpp, include/cSim3Solver.h) over mcs_sim3_*.  KF: the caller's keyframe type with GetMapPointMatches() (a vector of MP*),
// GetKeyPoint(i).octave, GetSigma2(level), keypoint_to_cam (find(i)->second) and camSystem (a cMultiCamSys_ of this header); MP: the map point type
// with isBad(), GetIndexInKeyFrame(KF*) (a vector of indices, the first is used) and GetWorldPos() (a Vec3d or anything indexable by 0..2).  The
// constructor's pointer filtering runs here, everything numeric on the device; the solver's RANSAC state lives in the library from its first iterate().
// The draws are the library's counter-based draws of `seed` (include/mcs_c.h: mcs_sim3_draw), not std::random_device's.
inline double Sim3At(const Vec3d& v, int i) { return v.v[i]; }
template <class T>
inline double Sim3At(const T& v, int i) { return (double)v[i]; }

template <class KF, class MP>
class cSim3Solver {
public:
	cSim3Solver(Context& ctx, KF* pKF1, KF* pKF2, const std::vector<MP*>& vpMatched12, cMultiCamSys_* camSys, uint64_t seed = 0)
	    : ctx_(ctx), cs_(camSys), seed_(seed), mN1_((int)vpMatched12.size()) {
		std::vector<MP*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
		for (int i1 = 0; i1 < mN1_; ++i1) {   // :71-134
			MP* pMP2 = vpMatched12[i1];
			if (!pMP2) continue;
			MP* pMP1 = vpKeyFrameMP1[i1];
			if (!pMP1) continue;
			if (pMP1->isBad() || pMP2->isBad()) continue;
			const auto idxs1 = pMP1->GetIndexInKeyFrame(pKF1);
			const auto idxs2 = pMP2->GetIndexInKeyFrame(pKF2);
			if (idxs1.empty() || idxs2.empty()) continue;
			const int indexKF1 = (int)idxs1[0], indexKF2 = (int)idxs2[0];
			if (indexKF1 < 0 || indexKF2 < 0) continue;
			sigma2_.push_back(pKF1->GetSigma2(pKF1->GetKeyPoint(indexKF1).octave));
			sigma2_.push_back(pKF2->GetSigma2(pKF2->GetKeyPoint(indexKF2).octave));
			cam_.push_back((int32_t)pKF1->keypoint_to_cam.find(indexKF1)->second);
			cam_.push_back((int32_t)pKF2->keypoint_to_cam.find(indexKF2)->second);
			const auto X1 = pMP1->GetWorldPos();
			const auto X2 = pMP2->GetWorldPos();
			for (int k = 0; k < 3; ++k) Xw_.push_back(Sim3At(X1, k));
			for (int k = 0; k < 3; ++k) Xw_.push_back(Sim3At(X2, k));
			index1_.push_back(i1);
		}
		const int nr = cs_->GetNrCams();
		for (KF* k : {pKF1, pKF2}) {
			const Matx44d inv = InvMat(k->camSystem.M_t);
			Mt_.insert(Mt_.end(), inv.begin(), inv.end());
		}
		for (KF* k : {pKF1, pKF2})
			for (int c = 0; c < nr; ++c) MtMc_.insert(MtMc_.end(), k->camSystem.MtMc_inv[c].begin(), k->camSystem.MtMc_inv[c].end());
		SetRansacParameters();
	}
	~cSim3Solver() { if (h_) mcs_sim3_destroy(h_); }
	cSim3Solver(const cSim3Solver&) = delete;
	cSim3Solver& operator=(const cSim3Solver&) = delete;

	void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {   // :139-165
		prob_ = probability; minInl_ = minInliers; maxIts_ = maxIterations;
		if (h_) mcs_throw(mcs_sim3_set_ransac_parameters(h_, &prob_, &minInl_, &maxIts_));
	}
	bool iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, Matx44d& result) {   // :167-254
		create();
		uint8_t ok = 0, noMore = 0;
		int32_t n = 0;
		std::vector<uint8_t> vb((size_t)std::max(mN1_, 1), 0);
		Matx44d T = result;
		mcs_throw(mcs_sim3_iterate(h_, &nIterations, &ok, &noMore, &n, T.data(), vb.data()));
		bNoMore = noMore != 0;
		nInliers = n;
		vbInliers.assign(mN1_, false);
		for (int i = 0; i < mN1_; ++i) vbInliers[i] = vb[i] != 0;
		if (ok) result = T;
		return ok != 0;
	}
	bool find(std::vector<bool>& vbInliers12, int& nInliers, Matx44d& result) {   // :256-262
		create();
		int32_t its = 0;
		mcs_throw(mcs_sim3_info(h_, nullptr, &its, nullptr));
		bool bFlag;
		return iterate(its, bFlag, vbInliers12, nInliers, result);
	}
	std::array<double, 9> GetEstimatedRotation() { std::array<double, 9> R{}; best(R.data(), nullptr, nullptr); return R; }
	Vec3d GetEstimatedTranslation() { Vec3d t{}; best(nullptr, t.v, nullptr); return t; }
	double GetEstimatedScale() { double s = 0; best(nullptr, nullptr, &s); return s; }
	int size() const { return (int)index1_.size(); }   // N: the correspondences the constructor kept

private:
	void create() {
		if (h_) return;
		std::vector<double> Mc;
		std::vector<mcs_ocam> oc;
		for (int c = 0; c < cs_->GetNrCams(); ++c) { Mc.insert(Mc.end(), cs_->M_c[c].begin(), cs_->M_c[c].end()); oc.push_back(cs_->camModels[c].ocam); }
		const int32_t off[2] = {0, (int32_t)index1_.size()};
		mcs_throw(mcs_sim3_create(ctx_.h, cs_->GetNrCams(), Mc.data(), oc.data(), 1, &mN1_, off, Mt_.data(), MtMc_.data(), &prob_, &minInl_, &maxIts_,
		                          Xw_.data(), cam_.data(), sigma2_.data(), index1_.data(), seed_, nullptr, &h_));
	}
	void best(double* R, double* t, double* s) { create(); mcs_throw(mcs_sim3_best(h_, R, t, s, nullptr, nullptr, nullptr)); }
	Context& ctx_;
	cMultiCamSys_* cs_;
	uint64_t seed_;
	int32_t mN1_;
	double prob_ = 0.99;
	int32_t minInl_ = 6, maxIts_ = 300;
	std::vector<double> Xw_, sigma2_, Mt_, MtMc_;
	std::vector<int32_t> cam_, index1_;
	mcs_sim3* h_ = nullptr;
};

// cLocalMapping::CreateNewMapPoints (src/cLocalMapping.cpp:223-381) over mcs_create_new_map_points: the current keyframe against its neighbours in the
// given order (GetBestCovisibilityKeyFrames), ONE device call — every neighbour is searched with the features that earlier neighbours gave a map point
// taken out.  KF: the caller's keyframe type with camSystem (a cMultiCamSys_ of this header), GetMapPointMatches() (a vector of MP*), GetKeyPoints() (a
// vector of 28-byte cv::KeyPoint-layout records), GetKeyPointsRays() (Vec3d or anything indexable by 0..2), keypoint_to_cam and
// cont_idx_to_local_cam_idx (find(i)->second), GetDescriptorRowPtr(cam, row) and, with havingMasks, GetDescriptorMaskRowPtr(cam, row)
// (src/cMultiKeyFrame.cpp:356-364); MP: GetWorldPos().  Per neighbour the accepted matches come back in the reference's order with their points; the
// map-point surgery (new cMapPoint, AddObservation, AddMapPoint, :362-368) stays with the caller; ComputeDistinctiveDescriptors / UpdateNormalAndDepth of the
// new points (:370-374) is cCovisibility::UpdateMapPoints once the caller has put their observations into the store.
struct NewMapPoints {
	struct Neighbour {
		std::vector<std::pair<size_t, size_t>> vMatchedIndices;   // accepted (idx1, idx2), ascending idx1
		std::vector<Vec3d> x3D;                                    // their points, world frame
		std::vector<int32_t> match12, verdict;                     // per feature of the current keyframe: the search's match, MCS_NP_*
		int nmatches = 0, fallbacks = 0;
		double baseline = 0, medianDepth = 0;
		bool skipped = false;                                      // baseline / medianDepth < 0.01 (:250-254)
	};
	std::vector<Neighbour> neighbours;
	std::vector<uint8_t> valid1;   // "has no map point yet" of the current keyframe after the loop
};

template <class KF, class MP>
NewMapPoints CreateNewMapPoints(Context& ctx, KF* pKF, const std::vector<KF*>& vpNeighKFs, bool checkOrientation = false, int descDim = 32,
                                bool havingMasks = false, double cosThresh = std::cos(3.0 * 3.14159265358979323846 / 180.0), double maxDIST = 25.0, int K = 16) {
	struct Flat {   // one keyframe as the call reads it
		std::vector<double> MtMc, MtMcInv, rays, mpPos;
		std::vector<mcs_ocam> cams;
		std::vector<mcs_keypoint> keys;
		std::vector<int32_t> cam, mpCam;
		std::vector<uint8_t> desc, mask, valid;
		mcs_kf_geom g{};
		mcs_desc_set d{};
	};
	auto flatten = [&](KF* kf, Flat& f, bool withMp) {
		cMultiCamSys_& cs = kf->camSystem;
		const int nr = cs.GetNrCams();
		for (int c = 0; c < nr; ++c) {
			f.MtMc.insert(f.MtMc.end(), cs.MtMc[c].begin(), cs.MtMc[c].end());
			f.MtMcInv.insert(f.MtMcInv.end(), cs.MtMc_inv[c].begin(), cs.MtMc_inv[c].end());
			f.cams.push_back(cs.camModels[c].ocam);
		}
		const auto keys = kf->GetKeyPoints();
		const auto rays = kf->GetKeyPointsRays();
		const std::vector<MP*> mps = kf->GetMapPointMatches();
		const size_t n = keys.size();
		f.keys.resize(n); f.cam.resize(n); f.valid.resize(n); f.rays.resize(3 * n);
		f.desc.resize(n * (size_t)descDim);
		if (havingMasks) f.mask.resize(n * (size_t)descDim);
		for (size_t i = 0; i < n; ++i) {
			static_assert(sizeof(keys[0]) == sizeof(mcs_keypoint), "GetKeyPoints() must hold cv::KeyPoint-layout records");
			std::memcpy(&f.keys[i], &keys[i], sizeof(mcs_keypoint));
			for (int k = 0; k < 3; ++k) f.rays[3 * i + k] = Sim3At(rays[i], k);
			const int c = (int)kf->keypoint_to_cam.find(i)->second, row = (int)kf->cont_idx_to_local_cam_idx.find(i)->second;
			f.cam[i] = c;
			std::memcpy(&f.desc[i * (size_t)descDim], kf->GetDescriptorRowPtr(c, row), (size_t)descDim);
			if (havingMasks) std::memcpy(&f.mask[i * (size_t)descDim], kf->GetDescriptorMaskRowPtr(c, row), (size_t)descDim);
			f.valid[i] = mps[i] ? 0 : 1;   // "if (pMP1) continue", src/cORBmatcher.cpp:1017-1020
			if (withMp && mps[i]) {
				const auto X = mps[i]->GetWorldPos();
				for (int k = 0; k < 3; ++k) f.mpPos.push_back(Sim3At(X, k));
				f.mpCam.push_back(c);
			}
		}
		f.g.MtMc = f.MtMc.data(); f.g.MtMc_inv = f.MtMcInv.data(); f.g.M_t = cs.M_t.data(); f.g.cams = f.cams.data();
		f.g.rays = f.rays.data(); f.g.keys = f.keys.data(); f.g.cam = f.cam.data(); f.g.n = (int32_t)n; f.g.nr_cams = nr;
		f.g.mp_pos = f.mpPos.data(); f.g.mp_cam = f.mpCam.data(); f.g.n_mp = (int32_t)f.mpCam.size();
		f.d.desc = f.desc.data(); f.d.mask = havingMasks ? f.mask.data() : nullptr; f.d.valid = f.valid.data(); f.d.group = f.cam.data();
		f.d.n = (int32_t)n; f.d.stride = descDim;
	};
	NewMapPoints out;
	const int ns = (int)vpNeighKFs.size();
	Flat cur;
	flatten(pKF, cur, false);
	const size_t n1 = (size_t)cur.g.n;
	out.valid1 = cur.valid;
	if (ns == 0) return out;
	std::vector<Flat> nb((size_t)ns);
	std::vector<mcs_kf_geom> g2((size_t)ns);
	std::vector<mcs_desc_set> d2((size_t)ns);
	for (int s = 0; s < ns; ++s) { flatten(vpNeighKFs[s], nb[s], true); g2[s] = nb[s].g; d2[s] = nb[s].d; }
	const size_t rows = std::max<size_t>(n1 * (size_t)ns, 1);
	std::vector<int32_t> verdict(rows), cnt((size_t)ns), a1(rows), a2(rows), m12(rows, -1), nm((size_t)ns), fb((size_t)ns);
	std::vector<double> x3D(3 * rows), ax(3 * rows), bl((size_t)ns), md((size_t)ns);
	std::vector<uint8_t> sk((size_t)ns), v1(std::max<size_t>(n1, 1));
	mcs_newpoints_out o{verdict.data(), x3D.data(), cnt.data(), a1.data(), a2.data(), ax.data()};
	mcs_throw(mcs_create_new_map_points(ctx.h, ns, &cur.g, &cur.d, g2.data(), d2.data(), nullptr, 0, descDim, K, checkOrientation ? 1 : 0, cosThresh, maxDIST,
	                                    MCS_MEM_HOST, m12.data(), nm.data(), fb.data(), bl.data(), md.data(), sk.data(), v1.data(), &o));
	out.valid1.assign(v1.begin(), v1.begin() + (std::ptrdiff_t)n1);
	out.neighbours.resize((size_t)ns);
	for (int s = 0; s < ns; ++s) {
		NewMapPoints::Neighbour& r = out.neighbours[s];
		const size_t lo = (size_t)s * n1;
		r.match12.assign(m12.begin() + (std::ptrdiff_t)lo, m12.begin() + (std::ptrdiff_t)(lo + n1));
		r.verdict.assign(verdict.begin() + (std::ptrdiff_t)lo, verdict.begin() + (std::ptrdiff_t)(lo + n1));
		r.nmatches = nm[s]; r.fallbacks = fb[s]; r.baseline = bl[s]; r.medianDepth = md[s]; r.skipped = sk[s] != 0;
		for (int k = 0; k < cnt[s]; ++k) {
			r.vMatchedIndices.emplace_back((size_t)a1[lo + k], (size_t)a2[lo + k]);
			r.x3D.push_back(Vec3d{{ax[3 * (lo + k)], ax[3 * (lo + k) + 1], ax[3 * (lo + k) + 2]}});
		}
	}
	return out;
}

// A camera system flattened for mcs_rig_view, with the image sizes mcs_frame_view carries (matrices = false: the sizes alone, the poses are not read).
struct FlatRig {
	std::vector<mcs_ocam> oc;
	std::vector<const uint8_t*> mm;
	std::vector<int32_t> w, h;
	std::vector<double> MtMc, MtMcInv;
	bool any = false;
	explicit FlatRig(cMultiCamSys_& cs, bool matrices = true) {
		for (int c = 0; c < cs.GetNrCams(); ++c) {
			cCamModelGeneral_& m = cs.camModels[c];
			oc.push_back(m.ocam); w.push_back(m.ocam.width); h.push_back(m.ocam.height);
			mm.push_back(m.mirrorMask0.empty() ? nullptr : m.mirrorMask0.data); any = any || !m.mirrorMask0.empty();
			if (!matrices) continue;
			MtMc.insert(MtMc.end(), cs.MtMc[c].begin(), cs.MtMc[c].end()); MtMcInv.insert(MtMcInv.end(), cs.MtMc_inv[c].begin(), cs.MtMc_inv[c].end());
		}
	}
	mcs_rig_view view() const { return mcs_rig_view{MtMcInv.data(), MtMc.data(), oc.data(), any ? mm.data() : nullptr, (int32_t)oc.size()}; }
};
// A frame flattened for mcs_tracked_frame / mcs_frame_view.  FR: mvKeys (28-byte cv::KeyPoint-layout records), keypoint_to_cam and cont_idx_to_local_cam_idx
// (find(i)->second), GetDescriptorRowPtr(cam, row) and, with havingMasks, GetDescriptorMaskRowPtr(cam, row).
struct FlatFrame {
	std::vector<mcs_keypoint> keys;
	std::vector<int32_t> cam;
	std::vector<uint8_t> desc, mask;
	int dim; bool masks;
	template <class FR>
	FlatFrame(const FR& F, int descDim, bool havingMasks) : dim(descDim), masks(havingMasks) {
		const size_t nf = F.mvKeys.size();
		keys.resize(nf); cam.resize(nf); desc.resize(nf * (size_t)descDim); mask.resize(havingMasks ? nf * (size_t)descDim : 0);
		for (size_t i = 0; i < nf; ++i) {
			static_assert(sizeof(F.mvKeys[0]) == sizeof(mcs_keypoint), "mvKeys must hold cv::KeyPoint-layout records");
			std::memcpy(&keys[i], &F.mvKeys[i], sizeof(mcs_keypoint));
			const int c = (int)F.keypoint_to_cam.find(i)->second, row = (int)F.cont_idx_to_local_cam_idx.find(i)->second;
			cam[i] = c;
			std::memcpy(&desc[i * (size_t)descDim], F.GetDescriptorRowPtr(c, row), (size_t)descDim);
			if (havingMasks) std::memcpy(&mask[i * (size_t)descDim], F.GetDescriptorMaskRowPtr(c, row), (size_t)descDim);
		}
	}
	// scales: mvScaleFactors of the frame (null, 0 where the call does not read them)
	mcs_frame_view view(uint8_t* assigned, const FlatRig& rig, const double* scales, size_t nlevels) const {
		return mcs_frame_view{keys.data(), desc.data(), masks ? mask.data() : nullptr, cam.data(), assigned, (int32_t)keys.size(), dim, (int32_t)rig.w.size(),
		                      rig.w.data(), rig.h.data(), scales, (int32_t)nlevels};
	}
};

// cTracking::SearchReferencePointsInFrustum (src/cTracking.cpp:953-1012) over mcs_search_local_points: the first loop (:957-976) runs here as written, then
// cMultiFrame::isInFrustum for every local point in every camera, the nToMatch gate and cORBmatcher::SearchByProjection(F, mvpLocalMapPoints, th) are ONE
// device call.  Afterwards the tracking fields and visible counts are written back onto the map points, F.mvpMapPoints is filled and the reference's value
// (matches of the first loop + the search's) is returned.  FR: the caller's frame type with camSystem (a cMultiCamSys_ of this header), mnId, mvpMapPoints
// (vector of MP*), mvKeys (28-byte cv::KeyPoint-layout records), keypoint_to_cam and cont_idx_to_local_cam_idx (find(i)->second), mvScaleFactors,
// GetDescriptorRowPtr(cam, row) and, with havingMasks, GetDescriptorMaskRowPtr(cam, row).  MP: GetWorldPos(), GetNormal(), GetMinDistanceInvariance(),
// GetMaxDistanceInvariance(), isBad(), IncreaseVisible(), mnLastFrameSeen, GetDescriptorPtr() / GetDescriptorMaskPtr() and the per-camera fields
// mbTrackInView, mTrackProjX, mTrackProjY, mnTrackScaleLevel, mTrackViewCos (indexable by camera, at least GetNrCams() entries: include/cMapPoint.h:101-105).
// UpdateReference and the IncreaseFound bookkeeping of TrackLocalMap stay with the caller; PoseOptimization is cOptimizer::PoseOptimization below.
template <class FR, class MP>
int SearchReferencePointsInFrustum(Context& ctx, FR& F, std::vector<MP*>& vpLocalMapPoints, double th = 3.0, double nnratio = 0.8, int descDim = 32,
                                   bool havingMasks = false) {
	cMultiCamSys_& cs = F.camSystem;
	const int nr = cs.GetNrCams();
	int nrMatches = 0;
	for (size_t i = 0; i < F.mvpMapPoints.size(); ++i) {   // :957-976
		MP* pMP = F.mvpMapPoints[i];
		if (!pMP) continue;
		if (pMP->isBad()) { F.mvpMapPoints[i] = nullptr; continue; }
		pMP->IncreaseVisible();
		pMP->mnLastFrameSeen = F.mnId;
		pMP->mbTrackInView[(int)F.keypoint_to_cam.find(i)->second] = false;
		++nrMatches;
	}
	const size_t np = vpLocalMapPoints.size(), ns = np * (size_t)nr;
	if (np == 0) return nrMatches;
	std::vector<double> pos(3 * np), nrm(3 * np), minD(np), maxD(np), px(ns), py(ns), vc(ns);
	std::vector<uint8_t> flags(np), inView(ns), desc(np * (size_t)descDim), mask(havingMasks ? np * (size_t)descDim : 0);
	std::vector<int32_t> lvl(ns), vis(np), match(ns, -1);
	for (size_t i = 0; i < np; ++i) {
		MP* pMP = vpLocalMapPoints[i];
		const auto X = pMP->GetWorldPos();
		const auto N = pMP->GetNormal();
		for (int k = 0; k < 3; ++k) { pos[3 * i + k] = Sim3At(X, k); nrm[3 * i + k] = Sim3At(N, k); }
		minD[i] = pMP->GetMinDistanceInvariance(); maxD[i] = pMP->GetMaxDistanceInvariance();
		flags[i] = (uint8_t)((pMP->isBad() ? MCS_LP_BAD : 0) | (pMP->mnLastFrameSeen == F.mnId ? MCS_LP_SEEN : 0));
		for (int c = 0; c < nr; ++c) {
			const size_t p = i * (size_t)nr + c;
			inView[p] = pMP->mbTrackInView[c] ? 1 : 0; px[p] = pMP->mTrackProjX[c]; py[p] = pMP->mTrackProjY[c];
			lvl[p] = pMP->mnTrackScaleLevel[c]; vc[p] = pMP->mTrackViewCos[c];
		}
		std::memcpy(&desc[i * (size_t)descDim], pMP->GetDescriptorPtr(), (size_t)descDim);
		if (havingMasks) std::memcpy(&mask[i * (size_t)descDim], pMP->GetDescriptorMaskPtr(), (size_t)descDim);
	}
	const FlatRig flatRig(cs);
	const FlatFrame frame(F, descDim, havingMasks);
	std::vector<uint8_t> assigned(std::max<size_t>(frame.keys.size(), 1));
	for (size_t i = 0; i < frame.keys.size(); ++i) assigned[i] = F.mvpMapPoints[i] ? 1 : 0;
	mcs_local_points lp{pos.data(), nrm.data(), minD.data(), maxD.data(), flags.data(), (int32_t)np};
	const mcs_rig_view rig = flatRig.view();
	mcs_track_state st{inView.data(), px.data(), py.data(), lvl.data(), vc.data()};
	const mcs_frame_view fv = frame.view(assigned.data(), flatRig, F.mvScaleFactors.data(), F.mvScaleFactors.size());
	int32_t nmatches = 0, nToMatch = 0;
	mcs_throw(mcs_search_local_points(ctx.h, &lp, &rig, &st, desc.data(), havingMasks ? mask.data() : nullptr, descDim, &fv, th, nnratio, descDim, MCS_MEM_HOST,
	                                  match.data(), &nmatches, &nToMatch, vis.data()));
	for (size_t i = 0; i < np; ++i) {
		MP* pMP = vpLocalMapPoints[i];
		for (int k = 0; k < vis[i]; ++k) pMP->IncreaseVisible();   // :995
		if (flags[i]) continue;                                    // the loop :981-999 never touched this point
		for (int c = 0; c < nr; ++c) {
			const size_t p = i * (size_t)nr + c;
			pMP->mbTrackInView[c] = inView[p] != 0; pMP->mTrackProjX[c] = px[p]; pMP->mTrackProjY[c] = py[p];
			pMP->mnTrackScaleLevel[c] = lvl[p]; pMP->mTrackViewCos[c] = vc[p];
		}
	}
	for (size_t p = 0; p < ns; ++p)
		if (match[p] >= 0) F.mvpMapPoints[(size_t)match[p]] = vpLocalMapPoints[p / (size_t)nr];   // F.mvpMapPoints[bestIdx] = pMP, src/cORBmatcher.cpp:159
	return nrMatches + nmatches;
}

// ---------------------------------------------------------------------------------------------- the frame-to-frame searches of cTracking
// mvpMapPoints as ids into per-point tables: ids are assigned from pointer identity in first-seen order
template <class MP>
struct PointIds {
	std::map<MP*, int32_t> id;
	std::vector<MP*> byId;
	std::vector<double> pos;
	std::vector<uint8_t> flags;
	std::vector<int32_t> of(const std::vector<MP*>& v) {
		std::vector<int32_t> out(v.size(), -1);
		for (size_t i = 0; i < v.size(); ++i) {
			MP* p = v[i];
			if (!p) continue;
			auto it = id.find(p);
			if (it == id.end()) {
				it = id.emplace(p, (int32_t)byId.size()).first;
				byId.push_back(p);
				const auto X = p->GetWorldPos();
				for (int k = 0; k < 3; ++k) pos.push_back(Sim3At(X, k));
				flags.push_back(p->isBad() ? MCS_LP_BAD : 0);
			}
			out[i] = it->second;
		}
		return out;
	}
	mcs_point_table table() const { return mcs_point_table{pos.data(), flags.data(), (int32_t)byId.size()}; }
};

// int cORBmatcher::SearchByProjection(cMultiFrame& CurrentFrame, const cMultiFrame& LastFrame, double th) (src/cORBmatcher.cpp:1990-2118), the search of
// cTracking::TrackWithMotionModel, as ONE device call (mcs_search_last_frame, host kind): CurrentFrame.mvpMapPoints is filled, the reference's value is
// returned.  FR additionally: camSystem (CurrentFrame), mvpMapPoints, mvbOutlier (LastFrame), mvScaleFactors (CurrentFrame).  MP: GetWorldPos(), isBad().
template <class FR, class MP>
int SearchByProjectionLastFrame(Context& ctx, FR& CurrentFrame, const FR& LastFrame, double th, int descDim = 32, bool havingMasks = false,
                                bool checkOrientation = false) {
	const FlatRig flatRig(CurrentFrame.camSystem);
	FlatFrame last(LastFrame, descDim, havingMasks), cur(CurrentFrame, descDim, havingMasks);
	const size_t nl = last.keys.size(), nc = cur.keys.size();
	PointIds<MP> ids;
	std::vector<int32_t> lastPoints = ids.of(LastFrame.mvpMapPoints), curPoints = ids.of(CurrentFrame.mvpMapPoints);
	std::vector<uint8_t> outlier(std::max<size_t>(nl, 1), 0), assigned(std::max<size_t>(nc, 1), 0);
	for (size_t i = 0; i < nl; ++i) outlier[i] = LastFrame.mvbOutlier[i] ? 1 : 0;
	for (size_t j = 0; j < nc; ++j) assigned[j] = CurrentFrame.mvpMapPoints[j] ? 1 : 0;
	mcs_tracked_frame tf{last.keys.data(), last.desc.data(), havingMasks ? last.mask.data() : nullptr, last.cam.data(), lastPoints.data(), outlier.data(), (int32_t)nl,
	                     descDim};
	const mcs_point_table tab = ids.table();
	const mcs_rig_view rig = flatRig.view();
	const mcs_frame_view fv = cur.view(assigned.data(), flatRig, CurrentFrame.mvScaleFactors.data(), CurrentFrame.mvScaleFactors.size());
	std::vector<int32_t> matchCur(std::max<size_t>(nc, 1), -1);
	int32_t nmatches = 0;
	mcs_throw(mcs_search_last_frame(ctx.h, &tf, &tab, &rig, &fv, th, descDim, checkOrientation ? 1 : 0, MCS_MEM_HOST, matchCur.data(), curPoints.data(), &nmatches));
	for (size_t j = 0; j < nc; ++j)
		if (matchCur[j] >= 0) CurrentFrame.mvpMapPoints[j] = LastFrame.mvpMapPoints[(size_t)matchCur[j]];   // :2075
	return nmatches;
}

// int cORBmatcher::WindowSearch(F1, F2, windowSize, vpMapPointMatches2, minScaleLevel, maxScaleLevel) (src/cORBmatcher.cpp:326-473), the first search of
// cTracking::TrackPreviousFrame, as ONE device call (mcs_window_search_frames, host kind).  vpMapPointMatches2 is rebuilt (F2.mvpMapPoints.size() entries, :333);
// nnratio is the matcher's mfNNratio.  FR: F2.camSystem gives the cameras and image sizes.
template <class FR, class MP>
int WindowSearchFrames(Context& ctx, FR& F1, FR& F2, int windowSize, std::vector<MP*>& vpMapPointMatches2, int minScaleLevel = 0, int maxScaleLevel = 0x7FFFFFFF,
                       double nnratio = 0.8, int descDim = 32, bool havingMasks = false, bool checkOrientation = false) {
	const FlatRig sizes(F2.camSystem, false);
	FlatFrame f1(F1, descDim, havingMasks), f2(F2, descDim, havingMasks);
	const size_t n1 = f1.keys.size(), n2 = f2.keys.size();
	PointIds<MP> ids;
	std::vector<int32_t> points1 = ids.of(F1.mvpMapPoints);
	mcs_tracked_frame tf{f1.keys.data(), f1.desc.data(), havingMasks ? f1.mask.data() : nullptr, f1.cam.data(), points1.data(), nullptr, (int32_t)n1, descDim};
	const mcs_point_table tab = ids.table();
	const mcs_frame_view fv = f2.view(nullptr, sizes, nullptr, 0);
	std::vector<int32_t> match21(std::max<size_t>(n2, 1), -1);
	int32_t nmatches = 0;
	mcs_throw(mcs_window_search_frames(ctx.h, &tf, &tab, &fv, windowSize, minScaleLevel, maxScaleLevel, nnratio, descDim, checkOrientation ? 1 : 0, MCS_MEM_HOST,
	                                   match21.data(), nullptr, &nmatches));
	vpMapPointMatches2.assign(F2.mvpMapPoints.size(), static_cast<MP*>(nullptr));   // :333
	for (size_t j = 0; j < n2 && j < vpMapPointMatches2.size(); ++j)
		if (match21[j] >= 0) vpMapPointMatches2[j] = F1.mvpMapPoints[(size_t)match21[j]];   // :428
	return nmatches;
}

// ---------------------------------------------------------------------------------------------- the frame's pose
// cOptimizer::PoseOptimization (src/cOptimizer.cpp:259-459) over mcs_pose_optimization (host kind), with the reference's signature: pFrame->mvbOutlier is
// written, the rig's pose is set through Set_M_t_from_min with the products the device built, `inliers` receives nBad / nInitialCorrespondences (the
// reference's out-parameter IS the outlier share) and nInitialCorrespondences - nBad is returned.  FR: camSystem (M_c_min filled, M_t_min = GetPoseMin()),
// mvKeys, keypoint_to_cam (find(i)->second), mvpMapPoints (vector of MP*), mvbOutlier, mvInvLevelSigma2.  MP: GetWorldPos(), isBad() (not read by the
// optimisation, as in the reference).  The batched form takes the frames of several candidates that share the rig model.
struct cOptimizer {
	template <class FR, class MP>
	static std::vector<int> PoseOptimizationBatch(Context& ctx, const std::vector<FR*>& frames, std::vector<double>& inliers, const std::vector<double>& huberMultiplier,
	                                              std::vector<mcs_pose_diag>* diag = nullptr) {
		const size_t np = frames.size();
		std::vector<int> ret(np, 0);
		inliers.assign(np, 0.0);
		if (np == 0) return ret;
		cMultiCamSys_& cs = frames[0]->camSystem;
		const size_t nr = (size_t)cs.GetNrCams();
		if (cs.M_c_min.size() != nr) throw std::runtime_error("PoseOptimization: camSystem.M_c_min is not set");
		PointIds<MP> ids;
		std::vector<std::vector<mcs_keypoint>> keys(np);
		std::vector<std::vector<int32_t>> cam(np), points(np);
		std::vector<std::vector<uint8_t>> out(np);
		std::vector<mcs_pose_frame> fr(np);
		std::vector<uint8_t*> outs(np);
		std::vector<double> pose(6 * np), McMin(6 * nr), MtMc(np * nr * 16), MtMcInv(np * nr * 16), share(np);
		std::vector<mcs_ocam> oc;
		for (size_t c = 0; c < nr; ++c) { oc.push_back(cs.camModels[c].ocam); std::copy(cs.M_c_min[c].begin(), cs.M_c_min[c].end(), McMin.begin() + 6 * c); }
		for (size_t p = 0; p < np; ++p) {
			FR& F = *frames[p];
			const size_t n = F.mvpMapPoints.size();
			keys[p].resize(n); cam[p].resize(n); out[p].assign(std::max<size_t>(n, 1), 0);
			for (size_t i = 0; i < n; ++i) {
				static_assert(sizeof(F.mvKeys[0]) == sizeof(mcs_keypoint), "mvKeys must hold cv::KeyPoint-layout records");
				std::memcpy(&keys[p][i], &F.mvKeys[i], sizeof(mcs_keypoint));
				cam[p][i] = (int32_t)F.keypoint_to_cam.find(i)->second;
			}
			points[p] = ids.of(F.mvpMapPoints);
			fr[p] = mcs_pose_frame{keys[p].data(), cam[p].data(), points[p].data(), (int32_t)n};
			outs[p] = out[p].data();
			std::copy(F.camSystem.M_t_min.begin(), F.camSystem.M_t_min.end(), pose.begin() + 6 * p);
		}
		const mcs_point_table tab = ids.table();
		const std::vector<double>& sigma = frames[0]->mvInvLevelSigma2;
		std::vector<double> huber(huberMultiplier);
		huber.resize(np, huber.empty() ? 1.0 : huber.back());
		std::vector<int32_t> nin(np);
		if (diag) diag->assign(np, mcs_pose_diag{});
		mcs_throw(mcs_pose_optimization(ctx.h, (int)np, fr.data(), &tab, McMin.data(), oc.data(), (int)nr, sigma.data(), (int)sigma.size(), huber.data(), MCS_MEM_HOST,
		                                pose.data(), MtMc.data(), MtMcInv.data(), outs.data(), nin.data(), share.data(), diag ? diag->data() : nullptr));
		for (size_t p = 0; p < np; ++p) {
			FR& F = *frames[p];
			for (size_t i = 0; i < F.mvpMapPoints.size(); ++i) F.mvbOutlier[i] = out[p][i] != 0;
			std::array<double, 6> m;
			std::copy(pose.begin() + 6 * p, pose.begin() + 6 * p + 6, m.begin());
			F.camSystem.Set_M_t_from_min(m, &MtMc[p * nr * 16], &MtMcInv[p * nr * 16]);   // :452
			inliers[p] = share[p];
			ret[p] = nin[p];
		}
		return ret;
	}
	template <class FR, class MP = typename std::remove_pointer<typename decltype(FR::mvpMapPoints)::value_type>::type>
	static int PoseOptimization(Context& ctx, FR* pFrame, double& inliers, const double& huberMultiplier = 1.0) {
		std::vector<double> share;
		const std::vector<int> r = PoseOptimizationBatch<FR, MP>(ctx, std::vector<FR*>{pFrame}, share, std::vector<double>{huberMultiplier});
		inliers = share[0];
		return r[0];
	}

	// cOptimizer::OptimizeSim3 (src/cOptimizerLoopStuff.cpp:58-264) over mcs_sim3_optimize (host kind), with the reference's signature: vpMatches1 is nulled
	// in place where the reference nulls it, g2oS12 receives the optimised estimate (and is left alone on the `return 0` path, :234-235), the inlier count is
	// returned.  KF: camSystem (a cMultiCamSys_ of this header; M_c and the cameras of pKF1 serve both sides, M_t of each), GetMapPointMatches() (a vector
	// of MP*), GetKeyPoint(i) (ptx, pty, octave), GetInvSigma2(level), GetSigma2(level), keypoint_to_cam (find(i)->second).  MP: isBad(),
	// GetIndexInKeyFrame(KF*) (a vector of indices, the first is used), GetWorldPos() (indexable by 0..2).  Reproduced: the information
	// of the second edge is GetSigma2, not its inverse (:188); e12 projects with pKF1's camera of feature i2 and e21 with pKF2's camera of feature i (the
	// point vertex an edge holds carries the other side's index).  Chosen: a match that pKF2 does not observe is skipped like i2 < 0 (the reference indexes
	// an empty vector); a crossed index that the other keyframe's keypoint_to_cam does not hold throws (the reference dereferences end()).
	struct Sim3 {   // g2o::Sim3: built from (R, t, s) as cLoopClosing::ComputeSim3 builds it; q (x y z w, not normalised) is set by an optimisation
		double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0}, s = 1.0, q[4] = {0, 0, 0, 1};
	};
	static double& stdSim() { static double v = 4.0; return v; }   // cOptimizer::stdSim (:55)
	template <class KF, class MP>
	static int OptimizeSim3(Context& ctx, KF* pKF1, KF* pKF2, std::vector<MP*>& vpMatches1, Sim3& g2oS12, mcs_sim3opt_diag* diag = nullptr) {
		cMultiCamSys_& cs = pKF1->camSystem;
		const size_t nr = (size_t)cs.GetNrCams();
		const std::vector<MP*> vpMapPoints1 = pKF1->GetMapPointMatches();
		std::vector<double> Xw, obs, w;
		std::vector<int32_t> cam;
		std::vector<size_t> at;
		for (size_t i = 0; i < vpMatches1.size(); ++i) {   // :117-199
			MP* pMP2 = vpMatches1[i];
			if (!pMP2) continue;
			MP* pMP1 = vpMapPoints1[i];
			const auto idx2 = pMP2->GetIndexInKeyFrame(pKF2);
			if (!pMP1 || idx2.empty() || pMP1->isBad() || pMP2->isBad() || (long long)idx2[0] < 0) continue;
			const size_t i2 = (size_t)idx2[0];
			const auto c1 = pKF1->keypoint_to_cam.find(i2), c2 = pKF2->keypoint_to_cam.find(i);
			if (c1 == pKF1->keypoint_to_cam.end() || c2 == pKF2->keypoint_to_cam.end()) throw std::runtime_error("OptimizeSim3: a crossed feature index has no camera");
			const auto X1 = pMP1->GetWorldPos();
			const auto X2 = pMP2->GetWorldPos();
			for (int k = 0; k < 3; ++k) Xw.push_back((double)X1[k]);
			for (int k = 0; k < 3; ++k) Xw.push_back((double)X2[k]);
			cam.push_back((int32_t)c1->second); cam.push_back((int32_t)c2->second);
			const auto k1 = pKF1->GetKeyPoint(i);
			const auto k2 = pKF2->GetKeyPoint(i2);
			obs.push_back((double)k1.ptx); obs.push_back((double)k1.pty); obs.push_back((double)k2.ptx); obs.push_back((double)k2.pty);
			w.push_back(pKF1->GetInvSigma2(k1.octave)); w.push_back(pKF2->GetSigma2(k2.octave));
			at.push_back(i);
		}
		const size_t n = at.size();
		std::vector<double> Mc(16 * nr), Mt(32);
		std::vector<mcs_ocam> oc;
		for (size_t c = 0; c < nr; ++c) { oc.push_back(cs.camModels[c].ocam); std::memcpy(&Mc[16 * c], cs.M_c[c].data(), 128); }
		const Matx44d i1 = InvMat(pKF1->camSystem.M_t), i2m = InvMat(pKF2->camSystem.M_t);
		std::memcpy(&Mt[0], i1.data(), 128); std::memcpy(&Mt[16], i2m.data(), 128);
		std::vector<uint8_t> keep(std::max<size_t>(n, 1), 1);
		uint8_t* keeps[1] = {keep.data()};
		const mcs_sim3opt_problem pr{n ? Xw.data() : nullptr, n ? cam.data() : nullptr, n ? obs.data() : nullptr, n ? w.data() : nullptr, (int32_t)n};
		const double std1 = stdSim();
		double S12[8], Ro[9];
		int32_t nin = 0;
		mcs_sim3opt_diag d{};
		mcs_throw(mcs_sim3_optimize(ctx.h, 1, &pr, Mc.data(), oc.data(), (int)nr, Mt.data(), &std1, g2oS12.R, g2oS12.t, &g2oS12.s, MCS_MEM_HOST, S12, Ro, keeps, &nin, &d));
		if (diag) *diag = d;
		for (size_t k = 0; k < n; ++k)
			if (!keep[k]) vpMatches1[at[k]] = nullptr;   // :219, :253
		if (d.status == MCS_SIM3OPT_OK && d.n_corr - d.n_bad1 >= 3) {   // :260-261; not on the return-0 path
			std::copy(S12, S12 + 4, g2oS12.q); std::copy(S12 + 4, S12 + 7, g2oS12.t); g2oS12.s = S12[7];
			std::copy(Ro, Ro + 9, g2oS12.R);
		}
		return nin;
	}

	// cOptimizer::LocalBundleAdjustment (src/cOptimizer.cpp:461-874) over mcs_local_bundle_adjustment (host kind), with the reference's signature less the map,
	// the iteration count and the covariance switch, which it does not read: builds lLocalKeyFrames, lLocalMapPoints and lFixedCameras and the fixing rules
	// (:473-529, :555-595), runs the call, applies the erasures (EraseMapPointMatch + EraseObservation), the bad flags, the positions and the poses, and returns
	// lLocalKeyFrames (empty when there is at most one, :489).  KF: mnId, isBad(), GetVectorCovisibleKeyFrames(), GetMapPointMatches() (vectors of pointers),
	// camSystem (a cMultiCamSys_ of this header: M_c_min, M_t_min, Set_M_t_from_min), keypoint_to_cam (find(i)->second), GetKeyPoint(i) (ptx, pty, octave),
	// mvInvLevelSigma2, EraseMapPointMatch(idx).  MP: isBad(), GetObservations() (a map KF* -> vector of feature indices), GetWorldPos() (indexable by 0..2),
	// SetWorldPos(const double*), EraseObservation(KF*, idx), SetBadFlag().  Where the reference iterates std::map<cMultiKeyFrame*, ...> the order here is
	// ascending mnId.  pbStopFlag as in the reference: g2o's terminate action WRITES it when round one converges and nothing is then written back (:756-762,
	// DESIGN.md section 7) — pass nullptr for the call that optimises.  UpdateNormalAndDepth / ComputeDistinctiveDescriptors of the written points (:866-867)
	// are the caller's (cCovisibility::UpdateMapPoints): `written`, optional, receives them.
	static double& stdRecon() { static double v = 2.0; return v; }   // cOptimizer::stdRecon
	template <class KF, class MP = typename std::remove_pointer<typename decltype(std::declval<KF>().GetMapPointMatches())::value_type>::type>
	static std::list<KF*> LocalBundleAdjustment(Context& ctx, KF* pKF, bool* pbStopFlag = nullptr, mcs_lba_diag* diag = nullptr, std::vector<MP*>* written = nullptr) {
		std::vector<KF*> local{pKF}, fixed;
		std::set<KF*> marked{pKF};
		for (KF* k : pKF->GetVectorCovisibleKeyFrames()) { marked.insert(k); if (!k->isBad()) local.push_back(k); }   // mnBALocalForKF is set on bad ones too (:484)
		if (local.size() <= 1) return std::list<KF*>();
		auto observations = [](MP* mp) {   // as std::map<cMultiKeyFrame*, ...> iterates: ascending mnId (the project's convention)
			std::vector<std::pair<KF*, std::vector<size_t>>> o;
			for (const auto& kv : mp->GetObservations()) o.emplace_back(kv.first, std::vector<size_t>(kv.second.begin(), kv.second.end()));
			std::stable_sort(o.begin(), o.end(), [](const std::pair<KF*, std::vector<size_t>>& a, const std::pair<KF*, std::vector<size_t>>& b) { return a.first->mnId < b.first->mnId; });
			return o;
		};
		std::vector<MP*> points;
		std::set<MP*> seen;
		for (KF* k : local)
			for (MP* mp : k->GetMapPointMatches())
				if (mp && !mp->isBad() && seen.insert(mp).second) points.push_back(mp);
		for (MP* mp : points)
			for (const auto& kv : observations(mp))
				if (marked.insert(kv.first).second && !kv.first->isBad()) fixed.push_back(kv.first);   // mnBAFixedForKF is set before the isBad test (:524-526)
		std::vector<KF*> kfs(local);
		kfs.insert(kfs.end(), fixed.begin(), fixed.end());
		std::vector<uint8_t> isFixed(kfs.size(), 1);
		bool oneFixed = false;
		for (size_t i = 0; i < local.size(); ++i) { oneFixed = local[i]->mnId == 0; isFixed[i] = oneFixed ? 1 : 0; }   // :564: overwritten per keyframe
		if (!oneFixed && fixed.empty()) isFixed[0] = 1;                                                                  // :575-581
		std::map<KF*, int32_t> slot;
		for (size_t i = 0; i < kfs.size(); ++i) slot[kfs[i]] = (int32_t)i;
		std::vector<int32_t> first{0}, ekf, ecam, total, badObs;
		std::vector<mcs_keypoint> keys;
		std::vector<std::pair<KF*, size_t>> at;
		std::vector<size_t> ptOf;
		std::vector<double> pos;
		for (size_t p = 0; p < points.size(); ++p) {
			int32_t t = 0, b = 0;
			for (const auto& kv : observations(points[p])) {
				t += (int32_t)kv.second.size();
				if (kv.first->isBad()) { b += (int32_t)kv.second.size(); continue; }
				for (size_t i : kv.second) {
					const auto kp = kv.first->GetKeyPoint(i);
					mcs_keypoint q{};
					q.x = kp.ptx; q.y = kp.pty; q.octave = kp.octave;
					keys.push_back(q);
					ekf.push_back(slot[kv.first]);
					ecam.push_back((int32_t)kv.first->keypoint_to_cam.find(i)->second);
					at.emplace_back(kv.first, i);
					ptOf.push_back(p);
				}
			}
			first.push_back((int32_t)ekf.size());
			total.push_back(t); badObs.push_back(b);
			const auto X = points[p]->GetWorldPos();
			for (int k = 0; k < 3; ++k) pos.push_back((double)X[k]);
		}
		cMultiCamSys_& cs = pKF->camSystem;
		const size_t nr = (size_t)cs.GetNrCams(), nl = local.size();
		if (cs.M_c_min.size() != nr) throw std::runtime_error("LocalBundleAdjustment: camSystem.M_c_min is not set");
		std::vector<double> pose(6 * kfs.size()), McMin(6 * nr), kfT(3 * nl);
		std::vector<mcs_ocam> oc;
		for (size_t c = 0; c < nr; ++c) { oc.push_back(cs.camModels[c].ocam); std::copy(cs.M_c_min[c].begin(), cs.M_c_min[c].end(), McMin.begin() + 6 * c); }
		for (size_t i = 0; i < kfs.size(); ++i) std::copy(kfs[i]->camSystem.M_t_min.begin(), kfs[i]->camSystem.M_t_min.end(), pose.begin() + 6 * i);
		std::vector<uint8_t> es(std::max<size_t>(ekf.size(), 1), 0), ps(std::max<size_t>(points.size(), 1), 1);
		first.resize(std::max<size_t>(first.size(), 1));
		int flag = pbStopFlag && *pbStopFlag ? 1 : 0;
		mcs_lba_diag d{};
		const std::vector<double>& sigma = pKF->mvInvLevelSigma2;
		mcs_throw(mcs_local_bundle_adjustment(ctx.h, (int)kfs.size(), (int)nl, pose.data(), isFixed.data(), kfT.data(), (int)points.size(), pos.data(), first.data(),
		                                      (int)ekf.size(), ekf.data(), ecam.data(), keys.data(), total.data(), badObs.data(), McMin.data(), oc.data(), (int)nr,
		                                      sigma.data(), (int)sigma.size(), stdRecon(), pbStopFlag ? &flag : nullptr, MCS_MEM_HOST, es.data(), ps.data(), &d));
		if (pbStopFlag) *pbStopFlag = flag != 0;
		if (diag) *diag = d;
		for (size_t e = 0; e < ekf.size(); ++e)
			if (es[e]) { at[e].first->EraseMapPointMatch(at[e].second); points[ptOf[e]]->EraseObservation(at[e].first, at[e].second); }   // :777-778, :810-811
		for (size_t p = 0; p < points.size(); ++p) {
			if (ps[p] == 2) points[p]->SetBadFlag();
			else if (ps[p] == 0) { points[p]->SetWorldPos(&pos[3 * p]); if (written) written->push_back(points[p]); }   // :865
		}
		if (d.status == MCS_LBA_OK)
			for (size_t i = 0; i < nl; ++i) {
				if (local[i]->isBad()) continue;
				std::array<double, 6> m;
				std::copy(pose.begin() + 6 * i, pose.begin() + 6 * i + 6, m.begin());
				local[i]->camSystem.Set_M_t_from_min(m);   // :833
			}
		return std::list<KF*>(local.begin(), local.end());
	}

	// cOptimizer::OptimizeEssentialGraph (src/cOptimizerLoopStuff.cpp:267-513) over mcs_optimize_essential_graph (host kind), with the reference's signature
	// (Scurw is not read there either): builds the vertex list without bad keyframes, the Sim3 of an uncorrected keyframe as Sim3(R, t, 1.0) of
	// GetPoseInverse() makes it (Eigen's Shoemake conversion, as csrc/mcs_sim3g.h restates it), the edge list in the reference's order with minNumFeat = 100
	// and the point references (:494-501), runs the call and applies SetPose and SetWorldPos.  A g2o::Sim3 is eight numbers in operator[] order, qx qy qz qw
	// tx ty tz s (EgSim3).  MAP: GetAllKeyFrames(), GetAllMapPoints() (vectors of pointers).  KF: mnId, isBad(), GetPoseInverse() (a Matx44d), GetParent(),
	// GetLoopEdges() and GetCovisiblesByWeight(w) (containers of KF*), GetWeight(KF*), SetPose(const Matx44d&).  MP: isBad(), GetWorldPos() (indexable by
	// 0..2), SetWorldPos(const double*), mnCorrectedByKF, mnCorrectedReference, GetReferenceKeyFrame().  Where the reference iterates a container ordered by
	// address (the keyframes, LoopConnections and its sets, GetLoopEdges) the order here is ascending mnId.  An edge that names a bad keyframe is left out
	// and a point whose reference keyframe has no vertex is left as it is.  UpdateNormalAndDepth of the moved points (:511) is the
	// caller's (cCovisibility::UpdateMapPoints): `moved`, optional, receives them.  Returns the call's status (MCS_EG_*); nothing is applied unless it is 0.
	using EgSim3 = std::array<double, 8>;
	static EgSim3 Sim3FromPose(const Matx44d& M) {   // Sim3(R, t, 1.0): Quaternion(const Matrix3d&), Geometry/Quaternion.h:720-759
		const double* R = M.data();
		auto m = [&](int i, int j) { return R[4 * i + j]; };
		EgSim3 S{};
		double t = m(0, 0) + (m(1, 1) + m(2, 2));
		if (t > 0.0) {
			t = std::sqrt(t + 1.0);
			S[3] = 0.5 * t;
			t = 0.5 / t;
			S[0] = (m(2, 1) - m(1, 2)) * t; S[1] = (m(0, 2) - m(2, 0)) * t; S[2] = (m(1, 0) - m(0, 1)) * t;
		} else {
			int i = 0;
			if (m(1, 1) > m(0, 0)) i = 1;
			if (m(2, 2) > m(i, i)) i = 2;
			const int j = (i + 1) % 3, k = (j + 1) % 3;
			t = std::sqrt(m(i, i) - m(j, j) - m(k, k) + 1.0);
			S[i] = 0.5 * t;
			t = 0.5 / t;
			S[3] = (m(k, j) - m(j, k)) * t;
			S[j] = (m(j, i) + m(i, j)) * t;
			S[k] = (m(k, i) + m(i, k)) * t;
		}
		S[4] = m(0, 3); S[5] = m(1, 3); S[6] = m(2, 3); S[7] = 1.0;
		return S;
	}
	template <class MAP, class KF, class MP = typename std::remove_pointer<typename decltype(std::declval<MAP>().GetAllMapPoints())::value_type>::type>
	static int OptimizeEssentialGraph(Context& ctx, MAP* pMap, KF* pLoopMKF, KF* pCurMKF, EgSim3& /*Scurw*/, const std::map<KF*, EgSim3>& NonCorrectedSim3,
	                                  const std::map<KF*, EgSim3>& CorrectedSim3, const std::map<KF*, std::set<KF*>>& LoopConnections, mcs_eg_diag* diag = nullptr,
	                                  std::vector<MP*>* moved = nullptr) {
		const int minNumFeat = 100;
		auto byId = [](std::vector<KF*> v) { std::stable_sort(v.begin(), v.end(), [](KF* a, KF* b) { return a->mnId < b->mnId; }); return v; };
		std::vector<KF*> kfs;
		for (KF* k : byId(pMap->GetAllKeyFrames()))
			if (!k->isBad()) kfs.push_back(k);
		std::map<KF*, int32_t> slot;
		for (size_t i = 0; i < kfs.size(); ++i) slot[kfs[i]] = (int32_t)i;
		const size_t K = kfs.size();
		std::vector<double> Scw(8 * K), Snc(8 * K, 0.0);
		std::vector<uint8_t> hasNc(K, 0), fixed(K, 0);
		for (size_t i = 0; i < K; ++i) {   // :305-342
			const auto c = CorrectedSim3.find(kfs[i]);
			const EgSim3 S = c != CorrectedSim3.end() ? c->second : Sim3FromPose(kfs[i]->GetPoseInverse());
			std::copy(S.begin(), S.end(), Scw.begin() + 8 * i);
			const auto n = NonCorrectedSim3.find(kfs[i]);
			if (n != NonCorrectedSim3.end()) { std::copy(n->second.begin(), n->second.end(), Snc.begin() + 8 * i); hasNc[i] = 1; }
			fixed[i] = kfs[i] == pLoopMKF ? 1 : 0;
		}
		std::vector<int32_t> ei, ej;
		std::vector<uint8_t> kind;
		auto edge = [&](KF* a, KF* b, uint8_t k) {
			const auto sa = slot.find(a), sb = slot.find(b);
			if (sa == slot.end() || sb == slot.end()) return;
			ei.push_back(sa->second); ej.push_back(sb->second); kind.push_back(k);
		};
		std::vector<KF*> heads;
		for (const auto& kv : LoopConnections) heads.push_back(kv.first);
		for (KF* k : byId(heads))   // :349-376
			for (KF* c : byId(std::vector<KF*>(LoopConnections.at(k).begin(), LoopConnections.at(k).end()))) {
				if ((k->mnId != pCurMKF->mnId || c->mnId != pLoopMKF->mnId) && k->GetWeight(c) < minNumFeat) continue;
				edge(k, c, 0);
			}
		for (KF* k : kfs) {   // :379-464
			if (KF* parent = k->GetParent()) edge(k, parent, 1);
			const auto loops = k->GetLoopEdges();
			for (KF* l : byId(std::vector<KF*>(loops.begin(), loops.end())))
				if (l->mnId < k->mnId) edge(k, l, 1);
			for (KF* c : k->GetCovisiblesByWeight(minNumFeat))
				if (c->mnId < k->mnId) edge(k, c, 1);
		}
		std::vector<MP*> points;
		for (MP* mp : pMap->GetAllMapPoints())
			if (mp && !mp->isBad()) points.push_back(mp);
		const size_t P = points.size();
		std::vector<double> pos(3 * std::max<size_t>(P, 1));
		std::vector<int32_t> ref(std::max<size_t>(P, 1), -1);
		for (size_t p = 0; p < P; ++p) {   // :494-501
			if ((long long)points[p]->mnCorrectedByKF == (long long)pCurMKF->mnId) {
				for (size_t i = 0; i < K; ++i)
					if ((long long)kfs[i]->mnId == (long long)points[p]->mnCorrectedReference) { ref[p] = (int32_t)i; break; }
			} else {
				const auto s = slot.find(points[p]->GetReferenceKeyFrame());
				if (s != slot.end()) ref[p] = s->second;
			}
			const auto X = points[p]->GetWorldPos();
			for (int k = 0; k < 3; ++k) pos[3 * p + k] = (double)X[k];
		}
		std::vector<double> out(8 * std::max<size_t>(K, 1)), pose(16 * std::max<size_t>(K, 1));
		mcs_eg_diag d{};
		mcs_throw(mcs_optimize_essential_graph(ctx.h, (int)K, Scw.data(), Snc.data(), hasNc.data(), fixed.data(), (int)ei.size(), ei.data(), ej.data(), kind.data(),
		                                       (int)P, pos.data(), ref.data(), MCS_MEM_HOST, out.data(), pose.data(), nullptr, &d));
		if (diag) *diag = d;
		if (d.status != MCS_EG_OK) return d.status;
		for (size_t i = 0; i < K; ++i) {   // :473-485
			Matx44d M;
			std::copy(pose.begin() + 16 * i, pose.begin() + 16 * i + 16, M.begin());
			kfs[i]->SetPose(M);
		}
		for (size_t p = 0; p < P; ++p)
			if (ref[p] >= 0) { points[p]->SetWorldPos(&pos[3 * p]); if (moved) moved->push_back(points[p]); }
		return d.status;
	}
};

// ---------------------------------------------------------------------------------------------- the local map and the covisibility counts
// cTracking::UpdateReferenceKeyFrames / UpdateReferencePoints (src/cTracking.cpp:1024-1123) and the counting and ordering of cMultiKeyFrame::UpdateConnections
// (src/cMultiKeyFrame.cpp:406-500), cLocalMapping::KeyFrameCulling / MapPointCulling (src/cLocalMapping.cpp:517-593, 187-221) over the device-resident
// observation store (mcs_covis_*).  KF: any type with `mnId`; map points are ids in [0, maxPoints),
// -1 where the reference holds NULL.  Where the reference orders by heap address the store orders by mnId.
template <class KF>
class cCovisibility {
public:
	struct Reference {   // what UpdateReferenceKeyFrames / UpdateReferencePoints leave on the tracker
		std::vector<KF*> mvpLocalKeyFrames; std::vector<int> mvpLocalKeyFramesCovWeights; std::vector<double> mvpLocalKeyFramesDistance2Frame;
		KF* mpReferenceKF = nullptr; std::vector<int32_t> mvpLocalMapPoints; int32_t nPoints = 0;   // nPoints > cap: the list was cut at cap
	};
	struct Connections {   // what UpdateConnections leaves on the keyframe; unchanged: KFcounter was empty, the reference keeps its old lists
		std::map<KF*, int> mConnectedKeyFrameWeights; std::vector<KF*> mvpOrderedConnectedKeyFrames; std::vector<int> mvOrderedWeights; bool unchanged = false;
	};
	cCovisibility(Context& ctx, int maxKeyFrames, int maxFeatures, int maxPoints) : maxPoints_(maxPoints) {
		mcs_throw(mcs_covis_create(ctx.h, maxKeyFrames, maxFeatures, maxPoints, &h_));
	}
	~cCovisibility() { if (h_) mcs_covis_destroy(h_); }
	cCovisibility(const cCovisibility&) = delete;
	cCovisibility& operator=(const cCovisibility&) = delete;

	void SetKeyFrame(KF* pKF, const std::vector<int32_t>& points) {
		const int64_t id = (int64_t)pKF->mnId;
		mcs_throw(mcs_covis_set_keyframe(h_, id, points.data(), (int)points.size(), MCS_MEM_HOST));
		if (!obj_.count(id)) slots_.push_back(pKF);
		obj_[id] = pKF;
	}
	void SetPose(KF* pKF, const double t[3]) { const int64_t id = (int64_t)pKF->mnId; mcs_throw(mcs_covis_set_keyframe_pose(h_, 1, &id, t, MCS_MEM_HOST)); }
	void EraseKeyFrame(KF* pKF) { mcs_throw(mcs_covis_erase_keyframe(h_, (int64_t)pKF->mnId)); }
	void SetBadFlag(KF* pKF, bool bad = true) { mcs_throw(mcs_covis_set_keyframe_bad(h_, (int64_t)pKF->mnId, bad ? 1 : 0)); }
	void SetPointsBad(const std::vector<int32_t>& ids, bool bad = true) {
		const std::vector<uint8_t> f(ids.size(), bad ? 1 : 0);
		mcs_throw(mcs_covis_set_points_bad(h_, ids.data(), (int)ids.size(), f.data(), MCS_MEM_HOST));
	}
	void clear() { mcs_throw(mcs_covis_clear(h_)); obj_.clear(); slots_.clear(); }
	int size() const { int n = 0; mcs_throw(mcs_covis_size(h_, &n)); return n; }
	int slots() const { int n = 0; mcs_throw(mcs_covis_slots(h_, &n)); return n; }

	// framePoints: mCurrentFrame.mvpMapPoints as ids, in/out (the entries of bad points become -1); frameT = Hom2T(mCurrentFrame.GetPose())
	Reference UpdateReference(std::vector<int32_t>& framePoints, const double frameT[3], int cap = -1) {
		const int S = slots();
		if (cap < 0) cap = maxPoints_;
		std::vector<int64_t> kfs((size_t)S + 1); std::vector<int32_t> w((size_t)S + 1), lp((size_t)cap + 1); std::vector<double> d((size_t)S + 1);
		int32_t nl = 0, np = 0; int64_t ref = -1;
		mcs_throw(mcs_covis_update_reference(h_, framePoints.data(), (int)framePoints.size(), frameT, cap, MCS_MEM_HOST, kfs.data(), w.data(), d.data(), &nl, &ref,
		                                     lp.data(), &np));
		Reference r;
		for (int k = 0; k < nl; ++k) { r.mvpLocalKeyFrames.push_back(obj_.at(kfs[k])); r.mvpLocalKeyFramesCovWeights.push_back(w[k]); r.mvpLocalKeyFramesDistance2Frame.push_back(d[k]); }
		r.mpReferenceKF = ref < 0 ? nullptr : obj_.at(ref);
		r.nPoints = np;
		r.mvpLocalMapPoints.assign(lp.begin(), lp.begin() + std::min(np, (int32_t)cap));
		return r;
	}
	Connections UpdateConnections(KF* pKF) { return UpdateConnections(std::vector<KF*>{pKF})[0]; }
	std::vector<Connections> UpdateConnections(const std::vector<KF*>& kfs) {   // the same calls one after another, in one device call
		const size_t nq = kfs.size(), S = (size_t)slots();
		std::vector<Connections> out(nq);
		if (!nq) return out;
		std::vector<int64_t> ids, od(nq * S); std::vector<int32_t> cnt(nq * S), nc(nq), ow(nq * S), no(nq);
		for (KF* k : kfs) ids.push_back((int64_t)k->mnId);
		mcs_throw(mcs_covis_update_connections(h_, (int)nq, ids.data(), MCS_MEM_HOST, cnt.data(), nc.data(), od.data(), ow.data(), no.data()));
		for (size_t q = 0; q < nq; ++q) {
			for (size_t k = 0; k < S; ++k)
				if (cnt[q * S + k] > 0) out[q].mConnectedKeyFrameWeights[slots_[k]] = cnt[q * S + k];
			out[q].unchanged = no[q] < 0;
			for (int k = 0; k < no[q]; ++k) { out[q].mvpOrderedConnectedKeyFrames.push_back(obj_.at(od[q * S + k])); out[q].mvOrderedWeights.push_back(ow[q * S + k]); }
		}
		return out;
	}
	// ---- cLocalMapping::KeyFrameCulling / MapPointCulling (src/cLocalMapping.cpp:517-593, 187-221)
	struct Culling {   // what KeyFrameCulling decided: SetBadFlag() these / mbToBeErased for these / the map points that went bad on the way
		std::vector<KF*> vpToSetBad, vpToBeErased; std::vector<int32_t> vBadPoints;
		std::vector<int32_t> verdict, nMPs, nRedundantObservations;   // per listed keyframe (verdict: 0 kept, 1 culled, 2 to be erased, 3 mnId == 0)
	};
	// octaves[i] = pKF->GetKeyPoint(i).octave
	void SetOctaves(KF* pKF, const std::vector<uint8_t>& octaves) {
		mcs_throw(mcs_covis_set_keyframe_octaves(h_, (int64_t)pKF->mnId, octaves.data(), (int)octaves.size(), MCS_MEM_HOST));
	}
	// vpLocalKeyFrames = mpCurrentMultiKeyFrame->GetVectorCovisibleKeyFrames(), in that order; notErase: mbNotErase per keyframe (empty: none).  Culled keyframes
	// and bad points are flagged in the store; the keyframes are NOT erased: the caller runs SetBadFlag() on vpToSetBad (spanning tree, mpMap, keyframe
	// database) and EraseKeyFrame() here.
	Culling KeyFrameCulling(const std::vector<KF*>& vpLocalKeyFrames, const std::vector<uint8_t>& notErase = std::vector<uint8_t>(), int cap = -1) {
		const size_t n = vpLocalKeyFrames.size();
		if (cap < 0) cap = maxPoints_;
		std::vector<int64_t> ids;
		for (KF* k : vpLocalKeyFrames) ids.push_back((int64_t)k->mnId);
		Culling r;
		r.verdict.assign(n + 1, 0); r.nMPs.assign(n + 1, 0); r.nRedundantObservations.assign(n + 1, 0);
		std::vector<int32_t> bp((size_t)cap + 1);
		int32_t nb = 0;
		mcs_throw(mcs_covis_cull_keyframes(h_, (int)n, ids.data(), notErase.size() == n && n ? notErase.data() : nullptr, cap, MCS_MEM_HOST, r.verdict.data(),
		                                   r.nMPs.data(), r.nRedundantObservations.data(), bp.data(), &nb));
		r.verdict.resize(n); r.nMPs.resize(n); r.nRedundantObservations.resize(n);
		for (size_t k = 0; k < n; ++k) {
			if (r.verdict[k] == 1) r.vpToSetBad.push_back(vpLocalKeyFrames[k]);
			if (r.verdict[k] == 2) r.vpToBeErased.push_back(vpLocalKeyFrames[k]);
		}
		r.vBadPoints.assign(bp.begin(), bp.begin() + std::min(nb, (int32_t)cap));
		return r;
	}
	// cMapPoint::Observations() of the listed points (0 for a bad one)
	std::vector<int32_t> Observations(const std::vector<int32_t>& points) {
		std::vector<int32_t> n(points.size());
		mcs_throw(mcs_covis_observations(h_, points.data(), (int)points.size(), MCS_MEM_HOST, n.data()));
		return n;
	}
	// recent = mlpRecentAddedMapPoints as ids (distinct), with mnFound / mnVisible / mnFirstKFid per entry; the points that stay remain in `recent`, the
	// verdicts (0 stays, 1 was bad, 2 / 3 SetBadFlag, 4 old enough) come back per entry of the list as it was
	std::vector<int32_t> MapPointCulling(KF* pCurrentKF, std::vector<int32_t>& recent, const std::vector<int32_t>& found, const std::vector<int32_t>& visible,
	                                     const std::vector<int64_t>& firstKFid) {
		std::vector<int32_t> v(recent.size());
		mcs_throw(mcs_covis_cull_points(h_, (int64_t)pCurrentKF->mnId, (int)recent.size(), recent.data(), found.data(), visible.data(), firstKFid.data(), MCS_MEM_HOST,
		                                v.data()));
		std::vector<int32_t> rest;
		for (size_t i = 0; i < recent.size(); ++i)
			if (v[i] == 0) rest.push_back(recent[i]);
		recent.swap(rest);
		return v;
	}
	// ---- cMapPoint::UpdateNormalAndDepth / ComputeDistinctiveDescriptors (src/cMapPoint.cpp:449-492, 294-388) for a list of map points
	struct MapPointUpdate {   // per listed point; status: 0 refreshed, 1 bad point, 2 reference keyframe not in the store, 3 level outside mvScaleFactors
		std::vector<int32_t> status, nDescriptors, bestFeature;   // an entry whose status is not 0 keeps what it held (zeros / -1 here)
		std::vector<double> mNormalVector, mfMinDistance, mfMaxDistance, minDistanceInvariance, maxDistanceInvariance;   // mNormalVector: 3 per point
		std::vector<KF*> bestKF;                                  // where the chosen descriptor lives; nullptr: none was chosen
	};
	// desc (/ mask): n rows of dim bytes, GetDescriptor(cam, idx) / GetDescriptorMask(cam, idx) in continuous feature-index order, one per entry of the
	// keyframe's row; mask may be nullptr.  The first call fixes dim and whether masks exist for the whole store.
	void SetDescriptors(KF* pKF, const uint8_t* desc, const uint8_t* mask, int dim, int n) {
		mcs_throw(mcs_covis_set_keyframe_descriptors(h_, (int64_t)pKF->mnId, desc, mask, dim, dim, n, MCS_MEM_HOST));
		dim_ = dim;
	}
	// points (distinct ids) with GetWorldPos() (3 doubles each) and mpRefKF per entry; scaleFactors = mvScaleFactors.  desc (/ mask): the points' current
	// descriptors, n rows of dim bytes, rewritten where one is chosen; desc == nullptr refreshes normal and depth only (cLoopClosing.cpp:511).
	MapPointUpdate UpdateMapPoints(const std::vector<int32_t>& points, const std::vector<double>& pos, const std::vector<KF*>& refKF,
	                               const std::vector<double>& scaleFactors, uint8_t* desc = nullptr, uint8_t* mask = nullptr) {
		const size_t n = points.size();
		MapPointUpdate r;
		r.status.assign(n + 1, 0); r.nDescriptors.assign(n + 1, 0); r.bestFeature.assign(n + 1, -1);
		r.mNormalVector.assign(3 * n + 1, 0.0); r.mfMinDistance.assign(n + 1, 0.0); r.mfMaxDistance.assign(n + 1, 0.0);
		r.minDistanceInvariance.assign(n + 1, 0.0); r.maxDistanceInvariance.assign(n + 1, 0.0);
		std::vector<int64_t> ref, best(n + 1, -1);
		for (KF* k : refKF) ref.push_back((int64_t)k->mnId);
		mcs_throw(mcs_covis_update_points(h_, (int)n, points.data(), pos.data(), ref.data(), scaleFactors.data(), (int)scaleFactors.size(), MCS_MEM_HOST,
		                                  r.mNormalVector.data(), r.mfMinDistance.data(), r.mfMaxDistance.data(), r.minDistanceInvariance.data(),
		                                  r.maxDistanceInvariance.data(), desc, mask, r.nDescriptors.data(), best.data(), r.bestFeature.data(), r.status.data()));
		r.status.resize(n); r.nDescriptors.resize(n); r.bestFeature.resize(n); r.mNormalVector.resize(3 * n); r.mfMinDistance.resize(n); r.mfMaxDistance.resize(n);
		r.minDistanceInvariance.resize(n); r.maxDistanceInvariance.resize(n);
		for (size_t i = 0; i < n; ++i) r.bestKF.push_back(best[i] < 0 ? nullptr : obj_.at(best[i]));
		return r;
	}
	int descriptorSize() const { return dim_; }
	mcs_covis* handle() const { return h_; }

private:
	mcs_covis* h_ = nullptr;
	int maxPoints_ = 0, dim_ = 0;
	std::map<int64_t, KF*> obj_;
	std::vector<KF*> slots_;   // slot -> keyframe, erased ones included (slot order is id order)
};

}  // namespace MultiColSLAM
