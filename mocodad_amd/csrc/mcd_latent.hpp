// mcd_latent.hpp -- what the host side (mcd_latent_api.hpp, inside mcd_api.hip) and the kernels (mcd_latent_kernel.hpp, inside
// mcd_latent.hip) of the MoCoDADlatent path share: sizes, the packed denoiser's description, launch parameters, launchers.
#pragma once
#include "mcd_device.hpp"

namespace mcd {

constexpr int LAT_MAX_LAYERS = 8;
constexpr int LAT_MAX_DIM = 128;          // D and every hidden size: a multiple of 16 in 16 .. 128
constexpr int LAT_NC = 32;                // chains (MFMA columns) a workgroup runs at a time: two n-tiles share every A fragment
constexpr int LAT_WAVES = 4;
constexpr int LAT_THREADS = LAT_WAVES * 64;
constexpr int LAT_HS = LAT_MAX_DIM + 4;   // row stride of the activation buffers (4 x odd: conflict-free ds_read_b128)
constexpr int LAT_MAX_S = 1024;           // per-sample losses of a workgroup's windows kept in LDS
constexpr int LAT_DOWN_LAYERS = 7;        // sp1a, sd1.0, sd1.1, sd2.0, sd2.1, sd3.0, sd3.1
constexpr int LAT_EMB = 400;              // emb_off(7): embedding outputs of the seven down-path layers
constexpr int LAT_ENC_C = 64;             // unet_down_channels[6] of the latent encoder (mocodad_latent.py:55)

// The denoiser in the packed buffer (offsets in floats).  Layer l: out = act(W' h + b') + (W_c e + b_c), act = ReLU behind the
// folded BatchNorm1d for all but the last layer, e = pos_encoding(i) + cond_emb.  Fragments: pack_gemm_frags order of
// [W_c | W'] (M = out, K = 16 + in): k-group 0 is the conditioning product, accumulated apart because the ReLU sits between.
struct LatentNet {
    int D, n_layers;
    int in[LAT_MAX_LAYERS], out[LAT_MAX_LAYERS];
    int wp[LAT_MAX_LAYERS], bias[LAT_MAX_LAYERS], cbias[LAT_MAX_LAYERS];
};

struct LatentChainParams {
    const float* wbuf;
    LatentNet net;
    const float* cond;        // (B,16); mode 1: (N,16)
    const float* z0;          // (B,D)
    const float* noise;       // parity mode: (S, max(ns-1,1), B, D); null: in-kernel Philox
    const float* step_table;  // (ns + 1, 4 + 16)
    const float* x_in;        // mode 1: (N,D)
    float* eps_out;           // mode 1: (N,D)
    float* loss_agg;          // (B,) or null
    float* loss_all;          // (B,S) or null
    float* latent_all;        // (B,S,D) or null
    float* latent_code;       // (B,D) or null
    unsigned long long seed;
    long long first_window;
    int B, S, ns, wpg;        // wpg: windows per workgroup (all their samples)
    int mode;                 // 0: chains; 1: one denoiser pass at step_single for B rows
    int step_single, loss_fn, aggr;
    float aggr_q;
};

// LDS plan of latent_chain_kernel for latent size D and chains_per_wg chains of a workgroup, offsets in floats: the kernel carves
// at them, launch_latent_chain asks for floats()
struct LatentChainLds {
    int XS, per_wg;           // row stride of X and Z0; per-sample losses kept
    __host__ __device__ LatentChainLds(int D, int chains_per_wg) : XS(D + 4), per_wg(chains_per_wg) {}
    __host__ __device__ int ha() const { return 0; }                              // activations, ping
    __host__ __device__ int hb() const { return ha() + LAT_NC * LAT_HS; }         // ... pong
    __host__ __device__ int x() const { return hb() + LAT_NC * LAT_HS; }          // chain state x[col][D]
    __host__ __device__ int z0() const { return x() + LAT_NC * XS; }              // latent code of the column's window
    __host__ __device__ int e() const { return z0() + LAT_NC * XS; }              // pos_encoding(i) + cond_emb [col][20]
    __host__ __device__ int ce() const { return e() + LAT_NC * 20; }              // cond_emb [col][16]
    __host__ __device__ int red() const { return ce() + LAT_NC * 16; }            // loss partial sums [col][8]
    __host__ __device__ int colb() const { return red() + LAT_NC * 8; }           // ints: window (mode 1: row) of a column, -1 = empty
    __host__ __device__ int cols() const { return colb() + LAT_NC; }              // ints: its sample
    __host__ __device__ int loss() const { return cols() + LAT_NC; }              // [window of the workgroup][S]
    __host__ __device__ int floats() const { return loss() + per_wg; }
};

// words of the packed buffer's offset table (mcd_device.hpp) that hold to_time_dim's weight / bias
constexpr int TAB_LAT_LW = 100, TAB_LAT_LB = 101;
// ... and, in an autoencoder handle (stage 'pretrain', pack_latent_ae_model) only: down1 / down2 once more in the CAPTURE k order
// (fragments + 0, 1; biases + 0, 1), whose B operands are the skip tensors d1 / d2 (resample_stage); rev_to_time_dim's weight as
// the A fragments of latent_unproject_kernel and its bias, both with the 640 t outputs in H's order [(t 10 + v) 64 + c].  The rows
// of layers 7 .. 10 (l * F_STRIDE), up3 / up2 (TAB_RSW / TAB_RSB + 2, 3) and the embedding rows 400 .. 529 of W_e are filled there too.
constexpr int TAB_LAT_CAPW = 102, TAB_LAT_CAPB = 104;
constexpr int TAB_LAT_RW = 106, TAB_LAT_RB = 107;

// launchers (mcd_latent.hip holds the kernels; mcd_api.hip only calls these)
// The rows of MCD_LATENT_ENCODE_INSTANCES this library holds: is there an encode kernel for t corrupt frames (cond_in_kernel: the
// fused form, the shipped condition encoder inside the launch); does its row compute z0 itself (false: it writes H and
// latent_project_kernel follows); the corrupt-frame counts of the rows, for messages ("3, 5, 6")
bool latent_encode_has_kernel(int t, bool cond_in_kernel);
bool latent_project_in_kernel(int t);
std::string latent_encode_counts();
// What a latent call derives from its cfg, view and step table, once (latent_call of mcd_latent_api.hpp), for the encode launches
// and the decode launch: the window view, the condition / corrupt frame lists, the table's row of the constant time step -1
struct LatentCall { DataView dv; FrameIdx cond_fi, fi; int seg_len; const float* pe_row; };
// cond_in_kernel = false: cond_out already holds cond_emb (B,16).  out: z0 (B,D), or H (B, 640 t) for a row that does not project
struct LatentEncodeArgs { const float* wbuf; const LatentCall& call; bool cond_in_kernel; float* cond_out; float* out; int D, B; hipStream_t st; };
int launch_latent_encode(int t, const LatentEncodeArgs& a);
// H (B, 640 t) -> z0 (B,D): to_time_dim of the rows with PROJECT_IN_KERNEL = false
int launch_latent_project(int t, const float* wbuf, const float* H, float* z0_out, int D, int B, hipStream_t st);
// The autoencoder's decoder half (mcd_latent_reconstruct).  z (B,D) -> G (B, 640 t) = rev_to_time_dim(z), in H's order
int launch_latent_unproject(int t, const float* wbuf, const float* z, float* G, int D, int B, hipStream_t st);
// is there a decode kernel for t corrupt frames (MCD_LATENT_DECODE_INSTANCES)
bool latent_decode_has_kernel(int t);
// G + the window's corrupt frames and cond_emb -> pose (B,2,t,17) and / or the window's mean loss against its corrupt frames (B)
struct LatentDecodeArgs { const float* wbuf; const LatentCall& call; const float* cond; const float* G; float* pose_out; float* loss_out; int loss_fn, B; hipStream_t st; };
int launch_latent_decode(int t, const LatentDecodeArgs& a);
// The same for the S generated latents of each window (mcd_latent_decode_samples): nb windows b0 .. b0 + nb - 1 of the call's B, G
// (nb S, 640 t) = the chunk's rows, window-major -> pose_all (B,S,2,t,17) (null: not wanted) and loss_all (B,S), both indexed by
// the call's window.  force_spw > 0: that many samples per workgroup (at most S) instead of the launcher's rule
// (latent_samples_per_wg in mcd_latent.hip); no result depends on it.
struct LatentDecodeSamplesArgs { const float* wbuf; const LatentCall& call; const float* cond; const float* G; float* pose_all; float* loss_all; int loss_fn, b0, nb, B, S, force_spw; hipStream_t st; };
int launch_latent_decode_samples(int t, const LatentDecodeSamplesArgs& a);
int launch_latent_chain(const LatentChainParams& P, hipStream_t st);
int launch_latent_philox(unsigned long long seed, long long first_window, int B, int S, int K, int D, float* out, hipStream_t st);

}  // namespace mcd
