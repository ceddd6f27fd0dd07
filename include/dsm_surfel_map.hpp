// dsm_surfel_map.hpp -- C++ host side above include/dsm_surfel_map.h with the reference's own class and
// method names, so that surfel_fusion/src/ros_node.cpp wires its subscribers to it unchanged:
//
//   reference (surfel_map.h:48-62)                                   this header
//   ---------------------------------------------------------------  ------------------------------------
//   SurfelMap(ros::NodeHandle &)   params of surfel_map.cpp:13-28     dsm::SurfelMap(const Params &)
//   image_input(const sensor_msgs::ImageConstPtr &)                   image_input(const ImagePtr &)
//   depth_input(const sensor_msgs::ImageConstPtr &)                   depth_input(const ImagePtr &)
//   orb_results_input(const sensor_msgs::PointCloudConstPtr &,        orb_results_input(const PointCloudPtr &,
//       const nav_msgs::PathConstPtr &, const nav_msgs::OdometryConstPtr &)   const PathPtr &, const OdometryPtr &)
//   save_map(const std_msgs::StringConstPtr &)                        save_map(const StringPtr &)
//   save_cloud(string) / save_mesh(string)                            save_cloud / save_mesh
//
// The callbacks are templates over the message pointer type: anything with the members the reference reads
// works -- the real ROS messages (header.stamp.sec/.nsec, width, height, step, encoding, data; channels[0].values;
// poses[i].pose; pose.pose, pose.covariance) when roscpp is present, or the plain structs of namespace
// dsm::msg below when it is not (this image has no ROS).  Images must already be mono8 / 32FC1: the reference
// converts with cv_bridge::toCvCopy (surfel_map.cpp:86,96), which is not part of this library.
// Errors: the reference returns void and prints; these throw std::runtime_error (-DDSM_NO_EXCEPTIONS: status).
#ifndef DSM_SURFEL_MAP_HPP
#define DSM_SURFEL_MAP_HPP

#include <cstdint>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "dsm_fusion_functions.hpp" // kDefaultEngineFlags
#include "dsm_surfel_map.h"

namespace dsm {

namespace msg { // ROS-free mirrors of the message fields the node reads
struct Time {
    uint32_t sec = 0, nsec = 0;
};
struct Header {
    uint32_t seq = 0;
    Time stamp;
    std::string frame_id;
};
struct Point {
    double x = 0, y = 0, z = 0;
};
struct Quaternion {
    double x = 0, y = 0, z = 0, w = 1;
};
struct Pose {
    Point position;
    Quaternion orientation;
};
struct PoseStamped {
    Header header;
    Pose pose;
};
struct PoseWithCovariance {
    Pose pose;
    double covariance[36] = {0};
};
struct Image { // sensor_msgs/Image
    Header header;
    uint32_t height = 0, width = 0;
    std::string encoding;
    uint8_t is_bigendian = 0;
    uint32_t step = 0;
    std::vector<uint8_t> data;
};
struct ChannelFloat32 {
    std::string name;
    std::vector<float> values;
};
struct PointCloud { // sensor_msgs/PointCloud: channels[0].values = flat pairs of keyframe indices
    Header header;
    std::vector<ChannelFloat32> channels;
};
struct Path { // nav_msgs/Path
    Header header;
    std::vector<PoseStamped> poses;
};
struct Odometry { // nav_msgs/Odometry: pose.covariance[0] > 0 = new keyframe, [1] = reference keyframe
    Header header;
    PoseWithCovariance pose;
};
struct String {
    std::string data;
};
typedef std::shared_ptr<const Image> ImageConstPtr;
typedef std::shared_ptr<const PointCloud> PointCloudConstPtr;
typedef std::shared_ptr<const Path> PathConstPtr;
typedef std::shared_ptr<const Odometry> OdometryConstPtr;
typedef std::shared_ptr<const String> StringConstPtr;
} // namespace msg

class SurfelMap {
  public:
    struct Params { // nh.getParam(...) of surfel_map.cpp:13-28
        int cam_width = 0, cam_height = 0;
        float cam_fx = 0, cam_fy = 0, cam_cx = 0, cam_cy = 0;
        float fuse_far_distence = 30.f, fuse_near_distence = 0.5f; // kitti_orb.launch:15-16
        int drift_free_poses = 10;
        bool rgbd = false;
        int device = 0;
        int surfel_capacity = 0;
        int max_buffered_frames = 0; // frames kept waiting for a pose: 0 = 5000 (ros_node.cpp:24-25), < 0 = unbounded (dsm_surfel_map.h)
        uint32_t engine_flags = kDefaultEngineFlags; // 0 or DSM_FLAG_EIGEN33_PRODUCTS (dsm_fusion_functions.hpp)
    };

    explicit SurfelMap(const Params &p) {
        dsm_surfel_map_config c = dsm_surfel_map_config();
        c.struct_size = sizeof c;
        c.cam_width = p.cam_width;
        c.cam_height = p.cam_height;
        c.cam_fx = p.cam_fx;
        c.cam_fy = p.cam_fy;
        c.cam_cx = p.cam_cx;
        c.cam_cy = p.cam_cy;
        c.fuse_far_distence = p.fuse_far_distence;
        c.fuse_near_distence = p.fuse_near_distence;
        c.drift_free_poses = p.drift_free_poses;
        c.rgbd = p.rgbd ? 1 : 0;
        c.device = p.device;
        c.surfel_capacity = p.surfel_capacity;
        c.max_buffered_frames = p.max_buffered_frames;
        c.engine_flags = p.engine_flags;
        own_pixels_ = (size_t)(p.cam_width > 0 ? p.cam_width : 0) * (size_t)(p.cam_height > 0 ? p.cam_height : 0);
        const int rc = dsm_surfel_map_create(&c, &m_);
        if (rc != DSM_OK) {
            m_ = nullptr;
#ifndef DSM_NO_EXCEPTIONS
            throw std::runtime_error(std::string("dsm::SurfelMap: ") + dsm_last_error(nullptr));
#endif
        }
    }
    SurfelMap(const SurfelMap &) = delete;
    SurfelMap &operator=(const SurfelMap &) = delete;
    ~SurfelMap() { dsm_surfel_map_destroy(m_); }

    // a colour camera's message (rgb8 / bgr8 / rgba8 / bgra8) goes to dsm_surfel_map_image_input_color, which converts it to grey
    // on the device with the weights of set_gray_weights -- what cv_bridge::toCvCopy(msg, MONO8) does on the reference's callback
    // thread (surfel_map.cpp:86); mono8, and anything else (refused), goes to dsm_surfel_map_image_input as before
    template <typename ImagePtr> int image_input(const ImagePtr &image_input) {
        const std::string &enc = image_input->encoding;
        if (enc == "rgb8" || enc == "bgr8" || enc == "rgba8" || enc == "bgra8")
            return check(dsm_surfel_map_image_input_color(m_, stamp_of(image_input->header.stamp), (int32_t)image_input->width,
                                                          (int32_t)image_input->height, (size_t)image_input->step, enc.c_str(),
                                                          image_input->data.data(), gray_weights_));
        return check(dsm_surfel_map_image_input(m_, stamp_of(image_input->header.stamp), (int32_t)image_input->width,
                                                (int32_t)image_input->height, (size_t)image_input->step,
                                                image_input->encoding.c_str(), image_input->data.data()));
    }
    // the grey weights of colour images: {wr, wg, wb, shift} of include/dsm.h's dsm_frame_format (DSM_GRAY_OPENCV_14BIT by default;
    // DSM_GRAY_OPENCV_15BIT for a cv_bridge built against OpenCV 4.x); a bad set is refused when the next colour image arrives
    void set_gray_weights(int32_t wr, int32_t wg, int32_t wb, int32_t shift) {
        gray_weights_[0] = wr; gray_weights_[1] = wg; gray_weights_[2] = wb; gray_weights_[3] = shift;
    }
    template <typename ImagePtr> int depth_input(const ImagePtr &depth_input) {
        return check(dsm_surfel_map_depth_input(m_, stamp_of(depth_input->header.stamp), (int32_t)depth_input->width,
                                                (int32_t)depth_input->height, (size_t)depth_input->step,
                                                depth_input->encoding.c_str(), depth_input->data.data()));
    }
    // a sensor's uint16 depth (16UC1: Kinect / RealSense drivers in millimetres -> (0.001f, DSM_DEPTH_U16_MULTIPLY); TUM PNGs ->
    // (5000, DSM_DEPTH_U16_DIVIDE)), converted to metres on the device -- no cv_bridge conversion on the callback thread
    template <typename ImagePtr> int depth_input_u16(const ImagePtr &depth_input, float scale, int op = DSM_DEPTH_U16_DIVIDE) {
        return check(dsm_surfel_map_depth_input_u16(m_, stamp_of(depth_input->header.stamp), (int32_t)depth_input->width,
                                                    (int32_t)depth_input->height, (size_t)depth_input->step, depth_input->encoding.c_str(),
                                                    reinterpret_cast<const uint16_t *>(depth_input->data.data()), scale, (int32_t)op));
    }
    template <typename PointCloudPtr, typename PathPtr, typename OdometryPtr>
    int orb_results_input(const PointCloudPtr &loop_stamp_input, const PathPtr &loop_path_input, const OdometryPtr &this_pose_input) {
        std::vector<dsm_pose_msg> path(loop_path_input->poses.size());
        for (size_t i = 0; i < path.size(); i++) path[i] = pose_of(loop_path_input->poses[i].pose);
        const dsm_pose_msg this_pose = pose_of(this_pose_input->pose.pose);
        double cov[36];
        for (int i = 0; i < 36; i++) cov[i] = this_pose_input->pose.covariance[i];
        static const float none = 0.f;
        const float *values = &none;
        int32_t n_values = 0;
        if (!loop_stamp_input->channels.empty() && !loop_stamp_input->channels[0].values.empty()) {
            values = loop_stamp_input->channels[0].values.data();
            n_values = (int32_t)loop_stamp_input->channels[0].values.size();
        }
        return check(dsm_surfel_map_orb_results_input(m_, stamp_of(loop_stamp_input->header.stamp), values, n_values, path.data(),
                                                      (int32_t)path.size(), stamp_of(this_pose_input->header.stamp), &this_pose, cov));
    }
    template <typename StringPtr> int save_map(const StringPtr &save_map_input) { return save_mesh(save_map_input->data); }
    int save_cloud(const std::string &save_path_name) { return check(dsm_surfel_map_save_cloud(m_, save_path_name.c_str())); }
    int save_mesh(const std::string &save_path_name) { return check(dsm_surfel_map_save_mesh(m_, save_path_name.c_str())); }

    // save_mesh's hexagons as a vertex buffer built on the GPU: six vertices per surfel in `layout` (36 floats per surfel for
    // DSM_MESH_VERTEX_REF6, 24 for DSM_MESH_VERTEX_XYZ_RGBA8 whose fourth is the bytes r g b 255); triangles: dsm_mesh_indices
    int get_mesh(dsm_mesh_vertex_layout layout, std::vector<float> &vertices) {
        const size_t per = layout == DSM_MESH_VERTEX_REF6 ? 36 : 24;
        int32_t n = 0;
        int rc = dsm_surfel_map_get_mesh(m_, layout, nullptr, 0, &n);
        while (rc == DSM_E_CAPACITY) {
            vertices.resize((size_t)n * per);
            rc = dsm_surfel_map_get_mesh(m_, layout, vertices.data(), n, &n);
        }
        if (rc == DSM_OK) vertices.resize((size_t)n * per);
        return check(rc);
    }
    int save_mesh_binary(const std::string &save_path_name) { return check(dsm_surfel_map_save_mesh_binary(m_, save_path_name.c_str())); }

    // the map as images (dsm_render_compose of dsm.h): what `camera` (nullptr: the node's) at `pose16` (cam -> world, column-major;
    // nullptr: the latest fuse's) sees of the surfels of cloud `kind`.  The planes that are not nullptr are resized to width * height
    // (normal: * 3) and filled: depth 0 / index -1 / normal 0 0 0 / intensity 0 where nothing is hit.
    int render(dsm_cloud_kind kind, const dsm_render_camera *camera, const float *pose16, uint32_t flags, std::vector<float> *depth,
               std::vector<int32_t> *index, std::vector<float> *normal, std::vector<uint8_t> *intensity, int32_t *n_surfels = nullptr) {
        const size_t px = camera ? (size_t)(camera->width > 0 ? camera->width : 0) * (size_t)(camera->height > 0 ? camera->height : 0) : own_pixels_;
        dsm_render_planes planes = {nullptr, nullptr, nullptr, nullptr};
        if (depth) { depth->resize(px); planes.depth = depth->data(); }
        if (index) { index->resize(px); planes.index = index->data(); }
        if (normal) { normal->resize(px * 3); planes.normal = normal->data(); }
        if (intensity) { intensity->resize(px); planes.intensity = intensity->data(); }
        int32_t n = 0;
        const int rc = check(dsm_surfel_map_render(m_, kind, camera, pose16, flags, &planes, &n));
        if (n_surfels) *n_surfels = n;
        return rc;
    }
    // the same into device memory of the node's GPU
    int render_device(dsm_cloud_kind kind, const dsm_render_camera *camera, const float *pose16, uint32_t flags, const dsm_render_planes &planes_device,
                      int32_t *n_surfels = nullptr) {
        int32_t n = 0;
        const int rc = check(dsm_surfel_map_render_device(m_, kind, camera, pose16, flags, &planes_device, &n));
        if (n_surfels) *n_surfels = n;
        return rc;
    }

    // the map as an occupancy voxel grid (dsm_grid_compose of dsm.h): the surfels of cloud `kind` in the grid `spec`.  The vectors that
    // are not nullptr are resized and filled: occupied / inflated to nz * ny * ((nx + 31) / 32) words, index to nz * ny * nx, cells
    // to the number of set voxels (of `inflated` with DSM_GRID_CELLS_OF_INFLATED): the voxel-down-sampled cloud as linear indices.
    int grid(dsm_cloud_kind kind, const dsm_grid_spec &spec, uint32_t flags, std::vector<uint32_t> *occupied, std::vector<uint32_t> *inflated,
             std::vector<int32_t> *index, std::vector<int32_t> *cells, int32_t *n_surfels = nullptr) {
        const size_t nx = spec.nx > 0 ? (size_t)spec.nx : 0, rows = (size_t)(spec.ny > 0 ? spec.ny : 0) * (size_t)(spec.nz > 0 ? spec.nz : 0);
        const size_t words = rows * ((nx + 31) / 32), vox = rows * nx;
        dsm_grid_planes planes = {nullptr, nullptr, nullptr, nullptr, 0};
        if (vox <= ((size_t)1 << 28)) { // (a larger grid is refused by the library; nothing is sized for it)
            if (occupied) { occupied->resize(words); planes.occupied = occupied->data(); }
            if (inflated) { inflated->resize(words); planes.inflated = inflated->data(); }
            if (index) { index->resize(vox); planes.index = index->data(); }
        }
        std::vector<int32_t> none(1);
        if (cells) { // count first, then fetch: the list is as long as the map is wide
            planes.cells = cells->empty() ? none.data() : cells->data();
            planes.cells_cap = (int32_t)(cells->size() < vox ? cells->size() : vox);
        }
        int32_t n = 0, n_cells = 0;
        int rc = dsm_surfel_map_grid(m_, kind, &spec, flags, &planes, &n, &n_cells);
        if (rc == DSM_E_CAPACITY && cells) {
            cells->resize((size_t)n_cells);
            planes.cells = cells->data();
            planes.cells_cap = n_cells;
            rc = dsm_surfel_map_grid(m_, kind, &spec, flags, &planes, &n, &n_cells);
        }
        if (rc == DSM_OK && cells) cells->resize((size_t)n_cells);
        if (n_surfels) *n_surfels = n;
        return check(rc);
    }
    // the same into device memory of the node's GPU
    int grid_device(dsm_cloud_kind kind, const dsm_grid_spec &spec, uint32_t flags, const dsm_grid_planes &planes_device, int32_t *n_surfels = nullptr,
                    int32_t *n_cells = nullptr) {
        int32_t n = 0, c = 0;
        const int rc = dsm_surfel_map_grid_device(m_, kind, &spec, flags, &planes_device, &n, &c);
        if (n_surfels) *n_surfels = n;
        if (n_cells) *n_cells = c;
        return check(rc);
    }

    // the map as a truncated Euclidean distance field (dsm_field_compose of dsm.h): the field, out to max_dist voxels, of the occupied
    // set that grid() gives for the same kind and spec.  The vectors that are not nullptr are resized to nz * ny * nx and filled.
    int field(dsm_cloud_kind kind, const dsm_grid_spec &spec, int32_t max_dist, uint32_t flags, std::vector<uint16_t> *dist2, std::vector<int32_t> *nearest,
              std::vector<float> *distance, int32_t *n_surfels = nullptr) {
        const size_t vox = (size_t)(spec.nx > 0 ? spec.nx : 0) * (size_t)(spec.ny > 0 ? spec.ny : 0) * (size_t)(spec.nz > 0 ? spec.nz : 0);
        dsm_field_planes planes = {nullptr, nullptr, nullptr};
        if (vox <= ((size_t)1 << 26)) { // (a larger grid is refused by the library; nothing is sized for it)
            if (dist2) { dist2->resize(vox); planes.dist2 = dist2->data(); }
            if (nearest) { nearest->resize(vox); planes.nearest = nearest->data(); }
            if (distance) { distance->resize(vox); planes.distance = distance->data(); }
        }
        int32_t n = 0;
        const int rc = dsm_surfel_map_field(m_, kind, &spec, max_dist, flags, &planes, &n);
        if (n_surfels) *n_surfels = n;
        return check(rc);
    }
    // the same into device memory of the node's GPU
    int field_device(dsm_cloud_kind kind, const dsm_grid_spec &spec, int32_t max_dist, uint32_t flags, const dsm_field_planes &planes_device,
                     int32_t *n_surfels = nullptr) {
        int32_t n = 0;
        const int rc = dsm_surfel_map_field_device(m_, kind, &spec, max_dist, flags, &planes_device, &n);
        if (n_surfels) *n_surfels = n;
        return check(rc);
    }

    // free and unknown space (dsm_grid_carve / dsm_grid_classify of dsm.h; the limits are stated in dsm_surfel_map.h): from the next
    // fuse on every fused frame is carved into a device bit set the node owns.  spec nullptr: off (the default).  A new spec, and
    // every loop-closure warp, clears the set; free_space_resets() counts the latter.
    int set_free_space(const dsm_grid_spec *spec, const dsm_carve_params *params = nullptr, uint32_t flags = 0) {
        return check(dsm_surfel_map_set_free_space(m_, spec, params, flags));
    }
    int64_t free_space_resets() const { return dsm_surfel_map_free_space_resets(m_); }
    // a copy of the accumulated set, [nz][ny][wx] words of the spec given to set_free_space (the caller sizes the memory)
    int free_space(uint32_t *free_out, int64_t *n_free = nullptr) { return check(dsm_surfel_map_free_space(m_, free_out, n_free)); }
    int free_space_device(void *free_device, int64_t *n_free = nullptr) { return check(dsm_surfel_map_free_space_device(m_, free_device, n_free)); }
    // the occupied set of grid(kind) in the accumulator's grid classified against the accumulated free set; planes in host memory
    int space(dsm_cloud_kind kind, const dsm_space_planes &planes, int32_t *n_surfels = nullptr, int32_t *n_frontier = nullptr) {
        return check(dsm_surfel_map_space(m_, kind, &planes, n_surfels, n_frontier));
    }
    int space_device(dsm_cloud_kind kind, const dsm_space_planes &planes_device, int32_t *n_surfels = nullptr, int32_t *n_frontier = nullptr) {
        return check(dsm_surfel_map_space_device(m_, kind, &planes_device, n_surfels, n_frontier));
    }
    // the frontier of space(kind) as connected clusters (dsm_frontier_query_init gives the query's defaults); table and label in host memory
    int frontier_clusters(dsm_cloud_kind kind, const dsm_frontier_query &query, dsm_component *table, int32_t table_cap, int32_t *label,
                          int32_t *n_clusters, int32_t *n_all = nullptr, int32_t *from_root = nullptr) {
        return check(dsm_surfel_map_frontier_clusters(m_, kind, &query, table, table_cap, label, n_clusters, n_all, from_root));
    }
    int frontier_clusters_device(dsm_cloud_kind kind, const dsm_frontier_query &query, dsm_component *table_device, int32_t table_cap, int32_t *label_device,
                                 int32_t *n_clusters, int32_t *n_all = nullptr, int32_t *from_root = nullptr) {
        return check(dsm_surfel_map_frontier_clusters_device(m_, kind, &query, table_device, table_cap, label_device, n_clusters, n_all, from_root));
    }
    // candidate poses (cam -> world, 16 column-major floats each) scored against space(kind): dsm_grid_view of dsm.h; view_query()
    // gives the query's defaults (the node's camera with the carve range, the frontier as target); scores and visible in host memory
    dsm_view_query view_query() const {
        dsm_view_query q;
        dsm_view_query_init(m_, &q);
        return q;
    }
    int view_gain(dsm_cloud_kind kind, const dsm_view_query &query, int32_t n_poses, const float *poses16, dsm_view_score *scores, uint32_t *visible = nullptr) {
        return check(dsm_surfel_map_view_gain(m_, kind, &query, n_poses, poses16, scores, visible));
    }
    int view_gain_device(dsm_cloud_kind kind, const dsm_view_query &query, int32_t n_poses, const float *poses16, dsm_view_score *scores_device,
                         uint32_t *visible_device = nullptr) {
        return check(dsm_surfel_map_view_gain_device(m_, kind, &query, n_poses, poses16, scores_device, visible_device));
    }
    // one carve of the latest fused frame into a caller's set in device memory: the stateless counterpart
    int carve_last(const dsm_grid_spec &spec, const dsm_carve_params *params, uint32_t flags, void *free_device) {
        return check(dsm_surfel_map_carve_last(m_, &spec, params, flags, free_device));
    }

    // the frame of the latest fuse aligned, point to plane, against the surfels of cloud `kind` seen from pose16_guess (cam -> world,
    // column-major; nullptr: the latest fuse's pose): dsm_align_frame of dsm.h.  params nullptr: dsm_align_params_init's defaults.
    // Nothing is changed: what to do with result.pose16 is the caller's decision.
    int align_last(dsm_cloud_kind kind, const float *pose16_guess, const dsm_align_params *params, dsm_align_result &result) {
        dsm_align_params own;
        if (!params) {
            dsm_align_params_init(&own);
            params = &own;
        }
        return check(dsm_surfel_map_align_last(m_, kind, pose16_guess, params, &result));
    }
    // the pose of the latest fuse, cam -> world, 16 column-major floats: align_last's default guess
    int last_pose16(float *pose16) { return check(dsm_surfel_map_last_pose16(m_, pose16)); }

    // the point-cloud topics (publish_*_pointcloud, surfel_map.cpp:1115-1151, 1283-1454): xyzi = 4 floats per point
    int get_cloud(dsm_cloud_kind kind, std::vector<float> &xyzi) {
        int32_t n = 0;
        int rc = dsm_surfel_map_get_cloud(m_, kind, nullptr, 0, &n);
        while (rc == DSM_E_CAPACITY) {
            xyzi.resize((size_t)n * 4);
            rc = dsm_surfel_map_get_cloud(m_, kind, xyzi.data(), n, &n);
        }
        if (rc == DSM_OK) xyzi.resize((size_t)n * 4);
        return check(rc);
    }
    // fn(publication) after every fuse, for the kinds in kinds_mask (DSM_CLOUD_BIT(kind) | ...); an empty fn or mask 0: off.
    // The publication's buffers are valid while fn runs.
    using PublishFn = std::function<void(const dsm_surfel_map_publication &)>;
    int set_publish(uint32_t kinds_mask, PublishFn fn) {
        if (!kinds_mask || !fn) {
            const int rc = dsm_surfel_map_set_publish(m_, 0, nullptr, nullptr);
            publish_.reset();
            return check(rc);
        }
        std::unique_ptr<PublishFn> next(new PublishFn(std::move(fn)));
        const int rc = dsm_surfel_map_set_publish(m_, kinds_mask, &SurfelMap::publish_trampoline, next.get());
        if (rc == DSM_OK) publish_ = std::move(next);
        return check(rc);
    }

    dsm_surfel_map *handle() const { return m_; }
    dsm_handle *engine() const { return dsm_surfel_map_engine(m_); }

  private:
    template <typename T> static dsm_stamp stamp_of(const T &t) {
        dsm_stamp s;
        s.sec = (uint32_t)t.sec;
        s.nsec = (uint32_t)t.nsec;
        return s;
    }
    template <typename P> static dsm_pose_msg pose_of(const P &p) {
        dsm_pose_msg o;
        o.px = p.position.x; o.py = p.position.y; o.pz = p.position.z;
        o.qx = p.orientation.x; o.qy = p.orientation.y; o.qz = p.orientation.z; o.qw = p.orientation.w;
        return o;
    }
    static void publish_trampoline(void *user, const dsm_surfel_map_publication *pub) { (*(PublishFn *)user)(*pub); }
    int check(int rc) {
#if !defined(DSM_NO_EXCEPTIONS) && !defined(DSM_WITH_ROS)
        if (rc != DSM_OK) throw std::runtime_error(std::string("dsm::SurfelMap: ") + dsm_surfel_map_last_error(m_));
#endif
        return rc; // (with DSM_WITH_ROS the callbacks report and carry on, as the reference's void callbacks do)
    }
    dsm_surfel_map *m_ = nullptr;
    size_t own_pixels_ = 0; // cam_width * cam_height: the size of render()'s planes for the node's own camera
    int32_t gray_weights_[4] = DSM_GRAY_OPENCV_14BIT;
    std::unique_ptr<PublishFn> publish_; // the callback: outlives the map (the destructor body destroys the map first)
};

} // namespace dsm

#ifdef DSM_WITH_ROS
// ---- the reference's class, signature for signature (surfel_map.h:48-62), for roscpp builds ------------------------
// `SurfelMap surfel_map(nh);` and the subscriber wiring of surfel_fusion/src/ros_node.cpp:22-32
//     nh.subscribe("image", 5000, &SurfelMap::image_input, &surfel_map);
//     sync.registerCallback(boost::bind(&SurfelMap::orb_results_input, &surfel_map, _1, _2, _3));
// bind to these members unchanged: they are plain (non-template, non-overloaded) member functions returning void.
// include/ros_compat/surfel_map.h puts this class behind the reference's own header name, so that ros_node.cpp
// compiles without an edit when that directory precedes the reference's src/ on the include path.
// Errors: the reference returns void and prints (surfel_map.cpp:31-32); so does this class (stderr), except that a
// constructor that cannot reach a gfx950 device throws std::runtime_error -- there is no CPU path to fall back to.
#include <cstdio>

#include <nav_msgs/Odometry.h>
#include <nav_msgs/Path.h>
#include <ros/ros.h>
#include <sensor_msgs/Image.h>
#include <sensor_msgs/PointCloud.h>
#include <std_msgs/String.h>

class SurfelMap {
  public:
    SurfelMap(ros::NodeHandle &_nh) : nh(_nh), impl_(params_from(_nh)) {}
    ~SurfelMap() {}

    void image_input(const sensor_msgs::ImageConstPtr &image_input) { report(impl_.image_input(image_input), "image_input"); }
    void depth_input(const sensor_msgs::ImageConstPtr &image_input) { report(impl_.depth_input(image_input), "depth_input"); }
    void set_gray_weights(int32_t wr, int32_t wg, int32_t wb, int32_t shift) { impl_.set_gray_weights(wr, wg, wb, shift); }
    void depth_input_u16(const sensor_msgs::ImageConstPtr &image_input, float scale, int op = DSM_DEPTH_U16_DIVIDE) {
        report(impl_.depth_input_u16(image_input, scale, op), "depth_input_u16");
    }
    void orb_results_input(const sensor_msgs::PointCloudConstPtr &loop_stamp_input, const nav_msgs::PathConstPtr &loop_path_input,
                           const nav_msgs::OdometryConstPtr &this_pose_input) {
        report(impl_.orb_results_input(loop_stamp_input, loop_path_input, this_pose_input), "orb_results_input");
    }
    void save_cloud(std::string save_path_name) { report(impl_.save_cloud(save_path_name), "save_cloud"); }
    void save_mesh(std::string save_path_name) { report(impl_.save_mesh(save_path_name), "save_mesh"); }
    void save_map(const std_msgs::StringConstPtr &save_map_input) { // surfel_map.cpp:75-81
        std::string save_name = save_map_input->data;
        printf("save mesh modelt to %s.\n", save_name.c_str());
        save_mesh(save_name);
        printf("save done!\n");
    }

    dsm::SurfelMap &engine_node() { return impl_; }

  private:
    // the nine parameters of surfel_map.cpp:14-29
    static dsm::SurfelMap::Params params_from(ros::NodeHandle &nh) {
        dsm::SurfelMap::Params p;
        bool get_all = true;
        get_all &= nh.getParam("cam_width", p.cam_width);
        get_all &= nh.getParam("cam_height", p.cam_height);
        get_all &= nh.getParam("cam_fx", p.cam_fx);
        get_all &= nh.getParam("cam_cx", p.cam_cx);
        get_all &= nh.getParam("cam_fy", p.cam_fy);
        get_all &= nh.getParam("cam_cy", p.cam_cy);
        get_all &= nh.getParam("fuse_far_distence", p.fuse_far_distence);
        get_all &= nh.getParam("fuse_near_distence", p.fuse_near_distence);
        get_all &= nh.getParam("drift_free_poses", p.drift_free_poses);
        if (!get_all) printf("ERROR! Do not have enough parameters!");
        else printf("fuse the distence between %4f m and %4f m.\n", p.fuse_near_distence, p.fuse_far_distence);
        return p;
    }
    void report(int rc, const char *what) {
        if (rc != DSM_OK) fprintf(stderr, "SurfelMap::%s: %s\n", what, dsm_surfel_map_last_error(impl_.handle()));
    }
    ros::NodeHandle &nh;
    dsm::SurfelMap impl_;
};
#endif // DSM_WITH_ROS
#endif
